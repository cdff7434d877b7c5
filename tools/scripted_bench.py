#!/usr/bin/env python3
"""Scripted-opponent measurement: ``cat_rollout_scripted`` against its torch form and against ``cat_act_step`` for the same rows, in one
process, the three alternating.

    python tools/scripted_bench.py [--envs 4096] [--rays 64 90] [--launches 500] [--reps 5] [--out profiles/scripted.txt]

Labyrinth 2v1 after a few random ticks; the three agents play "chase", "chase", "evade" (G = 3 rows per env).  Per ray count, device events
around ``--launches`` back-to-back launches on one stream, per launch: ``kernel_us`` (the scripted kernel), ``torch_us`` (``scripted_step``
on the GPU over the same buffers), ``act_step_us`` (``cat_act_step``, freshly seeded networks, the same rows), and ``kernel_gbps`` = the
``G * N * (3R + 36)`` bytes a launch must move (2R of distances, R of types, 4 of the uniform number, 16 + 16 of the state) over ``kernel_us``.
Back-to-back launches of a few microseconds include the gaps between them: these are per-launch figures of a stream, not kernel times.
``kernel_graph_us`` / ``kernel_graph_gbps``: the same launch 100 times in ONE captured graph, per launch over 20 replays -- no host call
between the launches, which is how the launch runs inside a captured rollout.
Before timing, the kernel's actions and state are checked against the torch form's on the timed buffers.  Needs a GPU; prints one JSON
line per ray count and appends them to ``--out`` when given."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from as_cops_and_thieves_amd import VecCopsEnv, load_preset  # noqa: E402
from as_cops_and_thieves_amd import _learn_native as ln  # noqa: E402
from as_cops_and_thieves_amd.selfplay.actor import PolicyActor  # noqa: E402
from as_cops_and_thieves_amd.selfplay.scripted import ScriptedActor, scripted_step  # noqa: E402


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


@torch.no_grad()
def measure(N: int, R: int, launches: int, reps: int) -> dict:
    env = VecCopsEnv(load_preset("labyrinth", 2, 1), N, num_rays=R, max_step_count=400, seed=1)
    env.reset()
    for t in range(5):
        env.step(env.random_actions(t))
    raw = env.raw_outputs()
    scripted = ScriptedActor(env, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"})
    policy = PolicyActor.from_checkpoint(None, env, fused=True)
    (grp,) = policy.groups.values()
    G = scripted.G
    params = ln.act_params({n: grp.policy.w(n) for n in ln.ACT_PARAM_NAMES})
    h, c = policy.state[grp.role]
    u = torch.rand(G, N, device="cuda")
    keep = torch.ones(N, device="cuda")
    sp = scripted.params
    d = raw["obs_distance"].transpose(0, 1).contiguous()
    t = raw["obs_type"].transpose(0, 1).contiguous()
    script, target = scripted._script_t, scripted._target_t
    state_t = torch.zeros_like(scripted.state)

    def kernel():
        ln.rollout_scripted(raw, scripted.indices, scripted.targets, scripted.table, u, keep, scripted.state, scripted.actions, sp.memory_ticks,
                            sp.clear_min, sp.turn_prob)

    def torch_form():
        scripted_step(d, t, u, state_t, keep.view(1, N), script, target, sp)

    def act_step():
        ln.act_step(raw, grp.indices, params, h[0], c[0], keep, u, policy.actions)

    scripted.state.zero_()
    kernel()
    want, new = scripted_step(d, t, u, state_t, keep.view(1, N), script, target, sp)
    torch.cuda.synchronize()
    assert torch.equal(scripted.actions.t(), want) and torch.equal(scripted.state, new), "the kernel differs from the torch form"
    res = {"envs": N, "rays": R, "rows": G * N, "launches": launches, "kernel_us": [], "torch_us": [], "act_step_us": []}
    for _ in range(reps):
        for name, fn in (("kernel_us", kernel), ("torch_us", torch_form), ("act_step_us", act_step)):
            res[name].append(round(per_launch_us(fn, launches), 2))
    res["kernel_graph_us"] = [round(graph_us(kernel), 2) for _ in range(reps)]
    res["median"] = {k: statistics.median(res[k]) for k in ("kernel_us", "torch_us", "act_step_us", "kernel_graph_us")}
    res["bytes"] = G * N * (3 * R + 36)
    res["kernel_gbps"] = round(res["bytes"] / (res["median"]["kernel_us"] * 1e-6) / 1e9, 1)
    res["kernel_graph_gbps"] = round(res["bytes"] / (res["median"]["kernel_graph_us"] * 1e-6) / 1e9, 1)
    env.check_errors()
    env.close()
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", type=int, nargs="+", default=[64, 90])
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    lines = [json.dumps(measure(args.envs, R, args.launches, args.reps)) for R in args.rays]
    for line in lines:
        print(line, flush=True)
    if args.out is not None:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
