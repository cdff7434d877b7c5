#!/usr/bin/env python3
"""Role-training measurement: the collect + update rate of a COP PHASE -- the cops' learner against a league of thief policies played by
``cat_act_league_step`` inside the rollout graph (``MAPPOTrainer.set_opponent``) -- with 1, 8 and 32 opponent segments, beside the
simultaneous mode's ``collect`` + ``update`` (both roles learn: two learners' worth of networks and updates in one stacked learner) on
the same shape and seeds, in one process, the forms taking turns.

    python tools/role_training_bench.py [--envs 4096] [--rays 64] [--horizon 128] [--rollouts 3] [--reps 5] [--segments 1,8,32]

Squarinth 2v1, fresh seeded weights, ``random_timesteps = learning_starts = 0`` so that every rollout is policy-driven and updated.  Per
form and repetition: wall time, ended by a device synchronise, of ``--rollouts`` x (``collect`` + ``update``) after two untimed rollouts
(the eager one and the capture) -> env-steps/s.  Reports every repetition, the median and the spread (min .. max).  Needs a GPU; prints
one JSON line."""
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
from as_cops_and_thieves_amd.selfplay.actor import LeagueActor  # noqa: E402
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig  # noqa: E402
from as_cops_and_thieves_amd.selfplay.self_play import even_segments  # noqa: E402


def build(args, segments):
    """segments == 0: the simultaneous mode (one stacked learner over both roles); otherwise a cop phase against that many thief segments."""
    env = VecCopsEnv(load_preset("squarinth", 2, 1), args.envs, num_rays=args.rays, max_step_count=400, seed=1)
    rc = RoleConfig(random_timesteps=0, learning_starts=0)
    tcfg = TrainerConfig(horizon=args.horizon, policy_freeze_duration=0, opponent_freeze_duration=0)
    tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, tcfg, seed=0, **({"split_roles": True} if segments else {}))
    if segments:
        actor = LeagueActor.from_env(env, segments, agents=["thief_0"], fused=True, seed=1)
        actor.set_matchups([(lo, hi, {"thief_0": s}) for s, (lo, hi) in enumerate(even_segments(args.envs, segments))])
        tr.set_opponent("thief", actor)
    torch.manual_seed(0)
    for _ in range(2):              # the eager rollout and the capture (and the update's own graphs)
        tr.collect()
        tr.update()
    torch.cuda.synchronize()
    return env, tr


def timed(tr, rollouts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rollouts):
        tr.collect()
        tr.update()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--rollouts", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segments", default="1,8,32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    forms = {"simultaneous": 0, **{f"cop_phase_{s}": int(s) for s in args.segments.split(",")}}
    built = {name: build(args, s) for name, s in forms.items()}
    steps = args.envs * args.horizon * args.rollouts
    res = {"envs": args.envs, "rays": args.rays, "horizon": args.horizon, "rollouts": args.rollouts, "reps": args.reps,
           "env_steps_per_s": {name: [] for name in forms}}
    for _ in range(args.reps):
        for name, (_, tr) in built.items():      # the forms take turns inside a repetition: drift hits all of them alike
            res["env_steps_per_s"][name].append(round(steps / timed(tr, args.rollouts)))
    res["median"] = {n: statistics.median(v) for n, v in res["env_steps_per_s"].items()}
    res["spread"] = {n: [min(v), max(v)] for n, v in res["env_steps_per_s"].items()}
    for env, _ in built.values():
        env.check_errors()
        env.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
