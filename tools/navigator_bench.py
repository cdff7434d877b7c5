#!/usr/bin/env python3
"""Navigator measurement: the map grids, ``cat_render_nav_build``, one ``cat_render_nav_step`` launch beside ``cat_rollout_scripted``'s, and
what the PRIVILEGED "pursue" / "flee" opponents (``selfplay/navigators.py``) are worth against the scripted and the random ones.

    python tools/navigator_bench.py [--envs 4096] [--launches 500] [--reps 5] [--episodes 256] [--out profiles/navigators.txt]

One JSON line per part:
* ``maps``: per bundled map at cell 16 and clearance 6 -- grid, free cells, the sizes of the connected components (NumPy; no GPU).
* ``build``: the labyrinth's table (3600 cells, 3600 workgroups) by device events around one launch, ``--reps`` times,
  and the time of ``navigation.hops_reference`` for the same table on the host.
* ``step``: labyrinth 2v1 x ``--envs`` after a few random ticks, cops pursue and the thief flees (G = 3 rows per env): device events around
  ``--launches`` back-to-back launches on one stream, per launch (``nav_us``), the same for ``cat_rollout_scripted`` with chase / chase /
  evade (``scripted_us``), and each launch 100 times in ONE captured graph, per launch over 20 replays (``*_graph_us``).  Back-to-back
  launches of a few microseconds include the gaps between them: these are per-launch figures of a stream, not kernel times.  Before timing
  the kernel's actions are checked against ``navigate_step`` on the timed buffers.
* ``matchups``: ``evaluate_against_navigators(env, None, episodes)`` on squarinth 2v1, 64 rays, max_step_count 400, the first episode of
  every slot, fixed seeds -- the shape of profiles/scripted.txt's purpose check -- plus chase v. evade played the same way for comparison.
Needs a GPU; appends the lines to ``--out`` when given."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from as_cops_and_thieves_amd import VecCopsEnv, load_preset  # noqa: E402
from as_cops_and_thieves_amd import _learn_native as ln  # noqa: E402
from as_cops_and_thieves_amd import navigation as nv  # noqa: E402
from as_cops_and_thieves_amd.maps import MAPS_DIR  # noqa: E402
from as_cops_and_thieves_amd.selfplay.navigators import NavigatorActor  # noqa: E402
from as_cops_and_thieves_amd.selfplay.scripted import ScriptedActor  # noqa: E402

GRAPH_LAUNCHES, GRAPH_REPLAYS = 100, 20


def graph_us(fn) -> float:
    """Per launch of ``fn`` when GRAPH_LAUNCHES of them replay as one captured graph."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_LAUNCHES):
            fn()
    for _ in range(3):
        graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(GRAPH_REPLAYS):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / (GRAPH_LAUNCHES * GRAPH_REPLAYS)


def per_launch_us(fn, launches: int) -> float:
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / launches


def maps_line() -> dict:
    out = {}
    for name in sorted(json.loads((MAPS_DIR / "presets.json").read_text())):
        free, Wc, Hc = nv.free_cells(load_preset(name).compile(), 16, 6.0)
        out[name] = {"grid": [Wc, Hc], "cells": Wc * Hc, "free": int(free.sum()), "components": nv.component_sizes(free, Wc, Hc),
                     "no_snap": int((nv.snap_cells(free, Wc, Hc) == nv.NONE).sum())}
    return {"part": "maps", "cell": 16, "clearance": 6.0, "maps": out}


def build_line(reps: int) -> dict:
    cm = load_preset("labyrinth").compile()
    free, Wc, Hc = nv.free_cells(cm, 16, 6.0)
    field = nv.NavField(16, [(free, Wc, Hc)], [], device="cuda")
    t0 = time.perf_counter()
    want = nv.hops_reference(free, Wc, Hc)
    host_s = time.perf_counter() - t0
    assert np.array_equal(field.hops_of(0), want), "the built table differs from hops_reference"
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ln.nav_build(field.grid_host, field.grid, field.free, field.hops)
        b.record()
        torch.cuda.synchronize()
        us.append(round(a.elapsed_time(b) * 1000.0, 1))
    reach = want[want != nv.NONE]
    return {"part": "build", "map": "labyrinth", "grid": [Wc, Hc], "workgroups": Wc * Hc, "free": int(free.sum()), "longest_path": int(reach.max()),
            "table_bytes": 2 * (Wc * Hc) ** 2, "build_us": us, "median_build_us": statistics.median(us), "hops_reference_host_s": round(host_s, 2)}


@torch.no_grad()
def step_line(N: int, launches: int, reps: int) -> dict:
    env = VecCopsEnv(load_preset("labyrinth", 2, 1), N, num_rays=64, max_step_count=400, seed=1)
    env.reset()
    for t in range(5):
        env.step(env.random_actions(t))
    raw = env.raw_outputs()
    nav = NavigatorActor(env, {"cop_0": "pursue", "cop_1": "pursue", "thief_0": "flee"})
    scripted = ScriptedActor(env, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"})
    u = torch.rand(3, N, device="cuda")
    keep = torch.ones(N, device="cuda")
    sp = scripted.params

    def nav_launch():
        ln.nav_step(raw["team_positions"], u, nav.field, nav.indices, nav.opponent_masks, nav.table, nav.actions, nav.nav_hops)

    def scripted_launch():
        ln.rollout_scripted(raw, scripted.indices, scripted.targets, scripted.table, u, keep, scripted.state, scripted.actions, sp.memory_ticks,
                            sp.clear_min, sp.turn_prob)

    nav_launch()
    want, hops = nv.navigate_step(raw["team_positions"], u, nav.field, nav.indices, nav._script_t, nav.opponent_masks)
    torch.cuda.synchronize()
    assert torch.equal(nav.actions.t(), want) and torch.equal(nav.nav_hops, hops), "the kernel differs from navigate_step"
    res = {"part": "step", "envs": N, "rows": 3 * N, "launches": launches, "nav_us": [], "scripted_us": []}
    for _ in range(reps):
        for name, fn in (("nav_us", nav_launch), ("scripted_us", scripted_launch)):
            res[name].append(round(per_launch_us(fn, launches), 2))
    res["nav_graph_us"] = [round(graph_us(nav_launch), 2) for _ in range(reps)]
    res["scripted_graph_us"] = [round(graph_us(scripted_launch), 2) for _ in range(reps)]
    res["median"] = {k: statistics.median(res[k]) for k in ("nav_us", "scripted_us", "nav_graph_us", "scripted_graph_us")}
    res["fallback_rows"] = int((hops < 0).sum())
    env.check_errors()
    env.close()
    return res


@torch.no_grad()
def matchups_line(E: int) -> dict:
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_against_navigators, evaluate_league
    env = VecCopsEnv(load_preset("squarinth", 2, 1), E, num_rays=64, max_step_count=400, seed=11)
    actor = LeagueActor.from_env(env, 1, fused=True)
    torch.manual_seed(12)
    res = evaluate_against_navigators(env, None, E, actor=actor)
    # the scripted pair on the same env and in the same way, for the comparison the navigators are for
    actor.set_matchups([(0, E, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"})])
    base = evaluate_league(env, actor)
    res["chase_vs_evade"] = {"cop_wins": base["cop_wins"][0], "thief_wins": base["thief_wins"][0], "timeouts": base["timeouts"][0],
                             "mean_length": float(base["length"].float().mean())}
    env.check_errors()
    env.close()
    return dict({"part": "matchups", "map": "squarinth", "roster": "2v1", "rays": 64, "max_step_count": 400, "env_seed": 11, "torch_seed": 12}, **res)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=256)
    ap.add_argument("--out", type=Path, default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    for part in (maps_line, lambda: build_line(args.reps), lambda: step_line(args.envs, args.launches, args.reps), lambda: matchups_line(args.episodes)):
        line = json.dumps(part())
        print(line, flush=True)
        if args.out is not None:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
