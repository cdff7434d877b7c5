#!/usr/bin/env python3
"""Frame skip, the three measurements of profiles/frame_skip.txt.

    python tools/frame_skip_bench.py [--envs 4096] [--maps labyrinth agh-map] [--ks 1 2 4 8] [--reps 30] [--out profiles/frame_skip.txt]
                                     [--bench-full] [--parent-bench FILE] [--regs-before FILE] [--regs-after FILE]
                                     [--trainer] [--frame-skips 1 2 4] [--rollouts 6]

1. Env alone: one `step_repeat(k)` launch against k `step_fused` launches on the same library.  Device events around each side, the two
   sides interleaved inside every repetition, a warm-up before the first, median and min .. max over the repetitions.  The repeat side's
   time is divided by the env ticks its slots actually played (the device sum of `ticks` over the interval / envs), the one-tick side's by
   k per decision; episodes are long (max_step_count 400), so nearly every slot plays all k ticks, and the mean played is printed too.
2. Defaults untouched (`--bench-full`): `python bench.py --full` of this tree is run `--bench-runs` times in child processes and its JSON
   lines are recorded; `--parent-bench FILE` holds the lines the same command printed on a checkout of the parent commit the same day and
   is copied beside them, as are the `tools/regs.sh` outputs of both commits (`--regs-before`, `--regs-after`).  What is not given is
   recorded as "not taken".
3. Trainer (`--trainer`): collect + update of `MAPPOTrainer` at `--envs` envs, 128-decision rollouts, `frame_skip` in `--frame-skips`:
   env-steps/s (from `read_stats()["env_ticks"]`) and decisions/s, wall clock around synchronised rollouts after two warm-up rollouts.
The header carries the env-core source hash (bench.source_sha16)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import torch
    from bench import source_sha16
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.sim import CatSim
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", nargs="+", default=["labyrinth", "agh-map"])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="decisions per timed interval")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_skip.txt"))
    ap.add_argument("--bench-full", action="store_true")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parent-bench", default=None)
    ap.add_argument("--regs-before", default=None)
    ap.add_argument("--regs-after", default=None)
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--frame-skips", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--rollouts", type=int, default=6)
    a = ap.parse_args()
    lines = [f"# frame skip, env alone: step_repeat(k) against k step_fused launches; source {source_sha16()}; {torch.cuda.get_device_name(0)}",
             f"# {a.envs} envs, 2v1, 64 rays; {a.reps} repetitions of {a.inner} decisions, sides interleaved; us per env tick: median (min .. max)"]
    for name in a.maps:
        sim = CatSim(SimConfig(n_envs=a.envs, n_rays=64, max_step_count=400, seed=1), [load_preset(name, 2, 1).compile()], device="cuda:0")
        sim.reset()
        acts = [sim.random_actions(t).clone() for t in range(a.inner)]
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for k in a.ks:
            played_sum = torch.zeros((), dtype=torch.int64, device="cuda:0")

            def repeat_side():
                played_sum.zero_()
                for x in acts:
                    played_sum.add_(sim.step_repeat(x, k)["ticks"].sum())
                return lambda: float(played_sum) / a.envs       # env ticks per slot actually played (read after the interval)
            def tick_side():
                for x in acts:
                    for _ in range(k):
                        sim.step_fused(x)
                return lambda: float(k * len(acts))
            for _ in range(3):
                repeat_side(); tick_side()
            res = {"repeat": [], "ticks": []}
            for _ in range(a.reps):
                for key, fn in (("repeat", repeat_side), ("ticks", tick_side)):
                    e0, e1 = ev(), ev()
                    e0.record(); n = fn(); e1.record()
                    torch.cuda.synchronize()
                    res[key].append(e0.elapsed_time(e1) * 1e3 / n())
            sim.step_repeat(acts[0], k)
            torch.cuda.synchronize()
            played = float(sim.out["ticks"].float().mean())
            fmt = lambda v: f"{statistics.median(v):7.2f} ({min(v):.2f} .. {max(v):.2f})"
            lines.append(f"{name:10s} k={k}: step_repeat {fmt(res['repeat'])}   k x step_fused {fmt(res['ticks'])}   mean ticks played {played:.3f}")
        assert sim.device_errors() == 0
        sim.close()
    lines += bench_section(a) + trainer_section(a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).write_text(text)


def bench_section(a):
    """Measurement 2: bench.py --full of this tree beside the parent's recorded lines, and the register records of both."""
    import subprocess
    out = ["", "## 2. defaults untouched: python bench.py --full, this commit and its parent"]
    if a.bench_full:
        for i in range(a.bench_runs):
            r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full"], capture_output=True, text=True, cwd=ROOT)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            out.append(f"this   run {i}: {line[-1] if r.returncode == 0 and line else 'FAILED rc=%d' % r.returncode}")
    else:
        out.append("this  : not taken (--bench-full)")
    for label, path in (("parent bench.py --full", a.parent_bench), ("tools/regs.sh before (parent)", a.regs_before), ("tools/regs.sh after (this)", a.regs_after)):
        if path:
            out += [f"# {label}:"] + Path(path).read_text().rstrip().splitlines()
        else:
            out.append(f"# {label}: not taken")
    return out


def trainer_section(a):
    """Measurement 3: collect + update at frame_skip in --frame-skips."""
    import time
    import torch
    out = ["", f"## 3. trainer: collect + update, {a.envs} envs, squarinth 2v1, 128-decision rollouts"]
    if not a.trainer:
        return out + ["not taken (--trainer)"]
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
    import dataclasses
    rc = dataclasses.replace(CFG_AGENT, random_timesteps=0, learning_starts=0)
    for k in a.frame_skips:
        env = VecCopsEnv(load_preset("squarinth"), a.envs, num_rays=64, max_step_count=400, seed=1)
        tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, TrainerConfig(horizon=128, frame_skip=k, policy_freeze_duration=0, opponent_freeze_duration=0), seed=0)
        for _ in range(2):
            tr.collect(); tr.update()
        torch.cuda.synchronize()
        t0_ticks, t0 = tr.read_stats()["env_ticks"], time.perf_counter()
        for _ in range(a.rollouts):
            tr.collect(); tr.update()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ticks = tr.read_stats()["env_ticks"] - t0_ticks
        out.append(f"frame_skip={k}: {ticks / dt / 1e6:8.3f} M env-steps/s   {a.rollouts * 128 * a.envs / dt / 1e6:8.3f} M decisions/s   "
                   f"({a.rollouts} rollouts in {dt:.3f} s)")
        env.check_errors()
        env.close()
    return out


if __name__ == "__main__":
    main()
