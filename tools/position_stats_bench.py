#!/usr/bin/env python3
"""What position tracking costs: labyrinth 2v1 x 4096 envs, 64 rays.

    python tools/position_stats_bench.py [--envs 4096] [--ticks 200] [--reps 8] [--out profiles/position_stats.txt]

1. Microseconds per env tick of a ``step_raw`` loop, timed with device events, in three configurations -- tracking off (the env as it
   was), occupancy only (``track_positions=8, position_exposure=False``), occupancy with exposure -- all in one process, their order
   alternating from repetition to repetition; medians and ranges over the repetitions.
2. The update kernel alone, at T = 1 (the env's current output buffers) and at T = 128 on ``rollout_fused`` rows, with and without
   obs_type: microseconds per launch and the achieved bytes per second against the A R + 4 A + 1 bytes per slot-row it must read
   (4 A + 1 without obs_type).
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=200, help="ticks of one timed loop")
    ap.add_argument("--reps", type=int, default=8, help="repetitions (at least 8)")
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.positions import PositionTracker
    if not torch.cuda.is_available():
        raise SystemExit("position_stats_bench needs a GPU")
    N, R, reps = args.envs, 64, max(8, args.reps)
    lines = [f"position statistics: labyrinth 2v1 x {N} envs, {R} rays, cell {args.cell}; {torch.cuda.get_device_name(0)}"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    configs = {"off": {}, "occupancy": {"track_positions": args.cell, "position_exposure": False}, "occupancy+exposure": {"track_positions": args.cell}}
    envs = {k: VecCopsEnv(load_preset("labyrinth", 2, 1), N, num_rays=R, max_step_count=400, seed=1, **kw) for k, kw in configs.items()}
    for e in envs.values():
        e.reset()
        for t in range(20):                                 # warm-up
            e.step_raw(e.random_actions(t))
    torch.cuda.synchronize()
    times, host = {k: [] for k in envs}, {k: [] for k in envs}
    names = list(envs)
    for r in range(reps):
        order = names[r % 3:] + names[:r % 3] if r % 2 == 0 else (names[r % 3:] + names[:r % 3])[::-1]
        for k in order:
            e = envs[k]
            acts = [e.random_actions(1000 + t).clone() for t in range(8)]
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            t0 = time.perf_counter()
            for t in range(args.ticks):
                e.step_raw(acts[t % 8])
            t1 = time.perf_counter()            # the host has queued every launch; the device may still be running them
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop) * 1e3 / args.ticks)
            host[k].append((t1 - t0) * 1e6 / args.ticks)
    say(f"step_raw loop, {args.ticks} ticks x {reps} repetitions, order alternating; microseconds per env tick of the batch")
    for k in names:
        v = times[k]
        say(f"  {k:<20} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   (host time to queue a tick: median "
            f"{statistics.median(host[k]):.2f}: the loop is host-bound where this equals the device figure)")
    base = statistics.median(times["off"])
    for k in names[1:]:
        say(f"  {k:<20} median - off median = {statistics.median(times[k]) - base:+.2f} us per tick")

    # the update kernel alone
    env = envs["off"]
    A = len(env.possible_agents)
    window = tuple(int(v) for v in env._compiled[0].window)
    say("update kernel alone (device events over 50 launches, median of 8); bytes = rows x N x (A R + 4 A + 1), 4 A + 1 without obs_type")
    for T in (1, 128):
        if T == 1:
            out = env.raw_outputs()
            rows = {k: out[k][None] for k in ("team_positions", "terminated", "obs_type")}
        else:
            rows = env._sim.rollout_fused(T, None, tick=5000, auto_reset=True)
        torch.cuda.synchronize()
        for with_obs in (False, True):
            tr = PositionTracker(N, env.possible_agents, 2, window, args.cell, device=env.device)
            obs = rows["obs_type"] if with_obs else None
            for _ in range(5):
                tr.update(rows["team_positions"], rows["terminated"], obs)
            torch.cuda.synchronize()
            us = []
            for _ in range(8):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(50):
                    tr.update(rows["team_positions"], rows["terminated"], obs)
                stop.record()
                stop.synchronize()
                us.append(start.elapsed_time(stop) * 1e3 / 50)
            nbytes = T * N * ((A * R if with_obs else 0) + 4 * A + 1)
            med = statistics.median(us)
            say(f"  T = {T:<4} {'with' if with_obs else 'without'} obs_type: median {med:8.2f} us per launch (min {min(us):.2f}, max {max(us):.2f}); "
                f"{nbytes} bytes -> {nbytes / med / 1e3:.2f} GB/s")
    for e in envs.values():
        e.check_errors()
        e.close()
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
