#!/usr/bin/env python3
"""League-pass measurement: ONE pass of S segments through ``cat_act_league_step`` against S plain passes of the same slots per
segment through ``cat_act_step``, in one process, the two forms alternating.

    python tools/act_league_bench.py [--segments 10] [--slots 5] [--rays 64] [--max-step-count 400] [--ticks 200] [--reps 5]

Labyrinth 2v1, fresh seeded weights (what an episode costs depends on how long the policies take to end it, not on the kernels).
(i) ``device_us``: device events around ``--ticks`` back-to-back act calls, per tick -- the league actor on S x slots rows, the plain
actor on ``slots`` rows ("plain"; the sequential form pays it S times per evaluated tick: "plain_x_S");
(ii) ``loop_s``: wall time, ended by a device synchronise, of the whole episode loop -- ``evaluate_league`` once on S x slots slots
against ``evaluate_agents`` S times on ``slots`` slots -- and the ticks each played.  Needs a GPU; prints one JSON line."""
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
from as_cops_and_thieves_amd.selfplay.actor import LeagueActor, PolicyActor  # noqa: E402
from as_cops_and_thieves_amd.selfplay.self_play import evaluate_agents, evaluate_league  # noqa: E402


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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--max-step-count", type=int, default=400)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    S, E = args.segments, args.slots
    preset = load_preset("labyrinth", 2, 1)
    big = VecCopsEnv(preset, S * E, num_rays=args.rays, max_step_count=args.max_step_count, seed=1)
    small = VecCopsEnv(preset, E, num_rays=args.rays, max_step_count=args.max_step_count, seed=1)
    agents = list(big.possible_agents)
    league = LeagueActor.from_env(big, S * len(agents), fused=True)
    league.set_matchups([(s * E, (s + 1) * E, {a: s * len(agents) + g for g, a in enumerate(agents)}) for s in range(S)])
    plain = PolicyActor.from_checkpoint(None, small, fused=True)
    for env in (big, small):
        env.reset()
    res = {"segments": S, "slots": E, "rays": args.rays, "max_step_count": args.max_step_count, "ticks": args.ticks,
           "device_us": {"league": [], "plain": []}, "loop_s": {"league": [], "sequential": []}, "loop_ticks": {"league": []}}
    for _ in range(args.reps):
        for name, actor, env in (("league", league, big), ("plain", plain, small)):
            starts = torch.zeros(env.num_envs, dtype=torch.bool, device="cuda")
            res["device_us"][name].append(round(device_us(actor, env, starts, args.ticks), 2))
    evaluate_league(big, league)                                 # both loops have run once before they are timed
    evaluate_agents(small, None, E, actor=plain)
    for rep in range(args.reps):
        torch.manual_seed(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evaluate_league(big, league)
        torch.cuda.synchronize()
        res["loop_s"]["league"].append(round(time.perf_counter() - t0, 4))
        res["loop_ticks"]["league"].append(out["ticks"])
        torch.manual_seed(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(S):
            evaluate_agents(small, None, E, actor=plain)
        torch.cuda.synchronize()
        res["loop_s"]["sequential"].append(round(time.perf_counter() - t0, 4))
    res["device_us_median"] = {n: statistics.median(v) for n, v in res["device_us"].items()}
    res["device_us_median"]["plain_x_S"] = round(res["device_us_median"]["plain"] * S, 2)
    res["loop_s_median"] = {n: statistics.median(v) for n, v in res["loop_s"].items()}
    for env in (big, small):
        env.check_errors()
        env.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
