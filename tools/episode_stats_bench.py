#!/usr/bin/env python3
"""What the on-device episode accounting (include/cat_episodes.h) costs, each figure against its yardstick in the same process.

1. ``cat_episodes_update`` at [T, N] = [1, 4096], [128, 4096], [1024, 4096], A = 3: device-event time per launch after warm-up,
   against the bytes it must move -- T * N * (4 A + 3) of streams plus the per-slot state read and written once -- at the rate of a
   1 GiB stream copy measured here (the measurement ``bench.py --full`` prints).  The T = 1 launch moves ~0.6 MB: it sits at the launch
   floor and is reported as a time, not a bandwidth.
2. The trainer's collect + update rate with ``TrainerConfig.episode_stats`` off and on: labyrinth 2v1, 4096 envs, 128-tick rollouts
   (the setting of ``bench.py``'s 128-tick learner leg), ``--reps`` repetitions of 5 timed rounds each, off and on alternating on
   trainers built once.  The spread of the off runs says whether the on figure differs.
3. Wall time of ``evaluate_agents`` against ``evaluate_agents_tracked`` at 512 envs on squarinth for 5 and 30 episodes, and the
   tracked function at 2048 episodes (the old one stops at one episode per slot).

    python tools/episode_stats_bench.py [--out profiles/episode_stats.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from as_cops_and_thieves_amd.environments import VecCopsEnv  # noqa: E402
from as_cops_and_thieves_amd.episodes import EpisodeTracker  # noqa: E402
from as_cops_and_thieves_amd.maps import load_preset  # noqa: E402
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig  # noqa: E402
from as_cops_and_thieves_amd.selfplay.self_play import evaluate_agents, evaluate_agents_tracked  # noqa: E402

AGENTS = ["cop_0", "cop_1", "thief_0"]


def stream_copy_rate(dev) -> float:
    """Bytes per second (read + write) of a 1 GiB device-to-device copy, as ``bench.py --full`` measures it."""
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize(dev)
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0.record()
    for _ in range(10):
        b.copy_(a)
    c1.record()
    torch.cuda.synchronize(dev)
    return 10 * 2 * a.numel() * 4 / (c0.elapsed_time(c1) * 1e-3)


def state_bytes(N: int, A: int) -> int:
    """The per-slot state, read and written once per launch: 3 f64 [A] vectors, 7 int32, 1 int64."""
    return 2 * N * (3 * 8 * A + 7 * 4 + 8)


def kernel_leg(dev, rate: float, iters: int, emit) -> None:
    N, A, msc = 4096, 3, 400
    emit(f"{'T':>5s} {'N':>5s} {'us/launch':>10s} {'MB moved':>9s} {'us at copy rate':>16s} {'GB/s':>8s} {'% of copy rate':>15s}")
    for T in (1, 128, 1024):
        g = torch.Generator(device="cpu").manual_seed(T)
        reward = torch.randn(T, N, A, generator=g).to(dev)
        term = (torch.rand(T, N, generator=g) < 1 / 60).to(torch.uint8)
        trunc = (term * (torch.rand(T, N, generator=g) < 0.3)).to(torch.uint8)
        winner = torch.where(term == 0, -1, torch.where(trunc == 1, 1, 0)).to(torch.int8)
        term, trunc, winner = term.to(dev), trunc.to(dev), winner.to(dev)
        tr = EpisodeTracker(N, AGENTS, msc, dev)
        for _ in range(5):
            tr.update(reward, term, trunc, winner)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            tr.update(reward, term, trunc, winner)
        e1.record()
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) * 1e3 / iters
        nbytes = T * N * (4 * A + 3) + state_bytes(N, A)
        floor_us = nbytes / rate * 1e6
        if T == 1:
            emit(f"{T:5d} {N:5d} {us:10.2f} {nbytes / 1e6:9.3f} {floor_us:16.3f} {'-':>8s} {'launch floor':>15s}")
        else:
            emit(f"{T:5d} {N:5d} {us:10.2f} {nbytes / 1e6:9.3f} {floor_us:16.3f} {nbytes / us / 1e3:8.1f} {100 * floor_us / us:15.1f}")


def trainer_leg(dev, reps: int, emit) -> None:
    rates = {False: [], True: []}
    trainers = {}
    for flag in (False, True):
        env = VecCopsEnv(load_preset("labyrinth"), num_envs=4096, num_rays=64, max_step_count=400, device=dev, track_episodes=flag)
        tr = MAPPOTrainer(env, None, TrainerConfig(horizon=128, episode_stats=flag), seed=0)
        for _ in range(3):                                     # the graphs are captured here
            tr.collect(); tr.update()
        torch.cuda.synchronize(dev)
        trainers[flag] = tr
    rounds = 5
    for _ in range(reps):
        for flag in (False, True):                             # alternating: both see the same neighbours on the box
            tr = trainers[flag]
            t0 = time.perf_counter()
            for _ in range(rounds):
                tr.collect(); tr.update()
            torch.cuda.synchronize(dev)
            rates[flag].append(rounds * 128 * 4096 / (time.perf_counter() - t0))
    off, on = rates[False], rates[True]
    emit(f"off: {' '.join(f'{v / 1e3:8.1f}' for v in off)}  k env-steps/s   median {statistics.median(off) / 1e3:.1f}, spread {min(off) / 1e3:.1f} .. {max(off) / 1e3:.1f}")
    emit(f"on : {' '.join(f'{v / 1e3:8.1f}' for v in on)}  k env-steps/s   median {statistics.median(on) / 1e3:.1f}, spread {min(on) / 1e3:.1f} .. {max(on) / 1e3:.1f}")
    inside = min(off) <= statistics.median(on) <= max(off)
    emit(f"median on / median off = {statistics.median(on) / statistics.median(off):.4f}; the on median lies "
         f"{'inside' if inside else 'OUTSIDE'} the spread of the off runs")
    stats = trainers[True].read_stats()
    emit(f"episodes accounted by the on trainer: {stats['episodes']}, cop win rate {stats['cop_win_rate']:.3f}, mean length {stats['mean_episode_length']:.1f}")
    for tr in trainers.values():
        tr.env.close()


def eval_leg(dev, emit) -> None:
    preset = load_preset("squarinth")
    rc = RoleConfig()
    tcfg = TrainerConfig(horizon=16, graph_rollout=False, graph_update=False)
    plain = VecCopsEnv(preset, 512, num_rays=64, max_step_count=2000, seed=3, device=dev)
    tracked = VecCopsEnv(preset, 512, num_rays=64, max_step_count=2000, seed=3, device=dev, track_episodes=True)
    runners = {False: MAPPOTrainer(plain, {"cop": rc, "thief": rc}, tcfg, seed=1), True: MAPPOTrainer(tracked, {"cop": rc, "thief": rc}, tcfg, seed=1)}

    def timed(flag, n):
        fn, env = (evaluate_agents_tracked, tracked) if flag else (evaluate_agents, plain)
        torch.manual_seed(11)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = fn(env, runners[flag], n)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, res

    timed(False, 5); timed(True, 5)                            # warm-up of every kernel of the tick
    emit(f"{'episodes':>8s} {'evaluate_agents s':>18s} {'tracked s':>10s} {'ratio':>6s}  results")
    for n in (5, 30):
        a, ra = timed(False, n)
        b, rb = timed(True, n)
        emit(f"{n:8d} {a:18.2f} {b:10.2f} {a / b:6.2f}  {ra} / {rb}")
    b, rb = timed(True, 2048)
    emit(f"{2048:8d} {'(one per slot only)':>18s} {b:10.2f} {'-':>6s}  {rb}; ticks played: {int(tracked.episode_tracker.per_slot()['len_sum'].max())}+")
    plain.close(); tracked.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="kernel,trainer,eval")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_stats_bench needs a GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s: str) -> None:
        print(s, flush=True)
        lines.append(s)
        if args.out:                                           # written as it grows: a leg that runs out of time keeps the ones before it
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    rate = stream_copy_rate(dev)
    emit(f"# episode_stats_bench: {torch.cuda.get_device_name(0)}; 1 GiB stream copy (read + write): {rate / 1e9:.0f} GB/s")
    if "kernel" in args.legs:
        emit(f"\n## 1. cat_episodes_update, A = 3, {args.iters} timed launches per row after 5 warm-up launches (device events)")
        kernel_leg(dev, rate, args.iters, emit)
    if "trainer" in args.legs:
        emit(f"\n## 2. trainer collect + update, labyrinth 2v1 x4096, 128-tick rollouts, {args.reps} repetitions x 5 rounds, off / on alternating")
        trainer_leg(dev, args.reps, emit)
    if "eval" in args.legs:
        emit("\n## 3. evaluation wall time, squarinth 2v1, 512 envs, max_step_count 2000, untrained networks, poll_every 32")
        eval_leg(dev, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
