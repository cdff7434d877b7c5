#!/usr/bin/env python3
"""Act-tick measurement: ``cat_act_step`` (one launch, include/cat_act.h) against the per-layer kernel chain it replaces, in ONE process.

    python tools/act_bench.py --rays 64 [--envs 4096] [--ticks 200] [--reps 5] [--row-tile 0]     # figures (i), (ii), (iv)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/act_bench.py --rays 64 --trace fused  # figure (iii), one run per back end
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/act_bench.py --rays 64 --trace chain

Labyrinth 2v1.  The yardstick is always the chain in the same process; chain and fused alternate, ``--reps`` repetitions each.
(i) time of one act tick by device events around ``--ticks`` back-to-back ``actor.act`` calls (no env step in between: the same
observations).  The chain's host work of a tick -- the observation dictionaries, ``stack``, ``torch.tensor`` -- lies inside that region, as it
does in every caller: where the host cannot keep the device busy the figure is the host's pace, not the sum of the kernels' times (that sum is
figure (iii), from the kernel trace);
(ii) eager wall time per tick of ``evaluate_agents``' loop, env step included; (iv) bytes allocated by a ``PolicyActor.from_checkpoint``
against a ``MAPPOTrainer`` at the default horizon.  ``--trace``: only 50 act ticks of one back end, for a kernel trace."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from as_cops_and_thieves_amd import VecCopsEnv, load_preset  # noqa: E402
from as_cops_and_thieves_amd.selfplay.actor import PolicyActor  # noqa: E402
from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig  # noqa: E402


@torch.no_grad()
def device_us(actor, env, starts, ticks):
    for _ in range(10):
        actor.act(env, starts)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ticks):
        actor.act(env, starts)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / ticks


@torch.no_grad()
def loop_us(actor, env, ticks):
    """``evaluate_agents``' tick: act, env.step, the winner book-keeping and its one host read."""
    obs, _ = env.reset()
    actor.reset()
    N = env.num_envs
    starts = torch.ones(N, dtype=torch.bool, device="cuda")
    winner = torch.full((N,), -1, dtype=torch.int8, device="cuda")
    open_ = torch.ones(N, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        actions = actor.act(env, starts, obs=obs)
        obs, _, terms, _, infos = env.step(actions)
        done = terms[actor.agents[0]]
        winner = torch.where(open_ & done, infos["winner"].to(torch.int8), winner)
        open_ = open_ & ~done
        starts = done.clone()
        bool(open_.any())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / ticks


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--row-tile", type=int, default=0)
    ap.add_argument("--trace", choices=["fused", "chain"], default=None)
    args = ap.parse_args()
    env = VecCopsEnv(load_preset("labyrinth", 2, 1), args.envs, num_rays=args.rays, max_step_count=2000, seed=1)
    env.reset()
    for t in range(20):
        env.step(env.random_actions(t))
    base = torch.cuda.memory_allocated()
    fused = PolicyActor.from_checkpoint(None, env, fused=True, row_tile=args.row_tile)
    actor_bytes = torch.cuda.memory_allocated() - base
    (grp,) = fused.groups.values()
    chain = PolicyActor([grp], fused.agents, fused.N, fused.R, fused.device, fused=False)     # the same parameters through the chain
    starts = torch.zeros(args.envs, dtype=torch.bool, device="cuda")
    if args.trace:
        a = fused if args.trace == "fused" else chain
        with torch.no_grad():
            for _ in range(50):
                a.act(env, starts)
        torch.cuda.synchronize()
        return 0
    res = {"rays": args.rays, "envs": args.envs, "ticks": args.ticks, "row_tile": args.row_tile, "device_us": {"chain": [], "fused": []},
           "loop_us": {"chain": [], "fused": []}}
    for _ in range(args.reps):
        for name, a in (("chain", chain), ("fused", fused)):
            res["device_us"][name].append(round(device_us(a, env, starts, args.ticks), 2))
    for _ in range(args.reps):
        for name, a in (("chain", chain), ("fused", fused)):
            res["loop_us"][name].append(round(loop_us(a, env, args.ticks), 2))
    for k in ("device_us", "loop_us"):
        res[k + "_median"] = {n: statistics.median(v) for n, v in res[k].items()}
    base = torch.cuda.memory_allocated()
    trainer = MAPPOTrainer(env, {"cop": CFG_AGENT, "thief": CFG_AGENT}, TrainerConfig(graph_rollout=False, graph_update=False))
    res["bytes"] = {"actor_allocated": actor_bytes, "actor_parameters": fused.parameter_bytes, "actor_state": fused.state_bytes,
                    "trainer_allocated": torch.cuda.memory_allocated() - base, "trainer_horizon": trainer.tcfg.horizon}
    env.check_errors()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
