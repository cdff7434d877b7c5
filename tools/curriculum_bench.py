#!/usr/bin/env python3
"""What the geodesic start-state curriculum (``TrainerConfig.spawn_curriculum``, ``cat_render_nav_spawn``) costs and does.  Each mode rewrites
its own section of the output file (default profiles/curriculum.txt) and keeps the others.  No threshold anywhere: the figures are written
down as measured.

    python tools/curriculum_bench.py resources [--parent-src PARENT]     # no GPU: registers of the kernels of cat_render.hip
    python tools/curriculum_bench.py fallback                            # no GPU: the share of slots the rule cannot place, per map and band
    python tools/curriculum_bench.py launch                              # GPU: a respawn per call, back to back and from a graph
    python tools/curriculum_bench.py trainer [--reps 7]                  # GPU: collect + update rate, option off / on
    python tools/curriculum_bench.py learning [--updates 150]            # GPU: cops against random thieves on squarinth, off / on

``resources``: ``-Rpass-analysis=kernel-resource-usage`` of cat_render.hip; with ``--parent-src`` (a checkout of the parent commit) the
other kernels' figures stand beside the parent's.
``fallback``: ``navigation.spawn_step`` on the arena field of each map, 2v1 x 4096 slots, all masked, at the bands the other modes use.
``launch``: labyrinth 2v1 x 4096 after 50 random ticks, about 1 % of the slots masked, band (2, 6): 200 ``respawn`` calls (the spawn kernel, the
counters' torch ops and the masked ``cat_reset``) back to back between two events, and a graph of 200 replayed, 7 times each; and the spawn
kernel alone.
``trainer``: squarinth 2v1 x 1024, horizon 64: one process, two trainers (off, on), legs alternating, each leg one collect() + update()
between two synchronisations; medians and ranges of ``--reps`` repetitions and the ratio to the OFF leg of the same run.
``learning``: squarinth 2v1 x 1024, horizon 128, thieves random (``random_action_roles``), ``--updates`` updates each, the same seed; then
every slot is turned off (``set_off``: the map's own spawn) and the cops' win rate is taken over ``--updates // 4`` more rollouts without an
update.  One run each: a figure, not a finding.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import geodesic_shaping_bench as gsb       # noqa: E402  (remarks, timed and the section writer are shared with the shaping profile)

SECTIONS = ("resources", "fallback", "launch", "trainer", "learning")
BAND, ADAPT, HI_MAX = (2, 6), (0.3, 0.7), 64


def resources(args) -> list:
    new = gsb.remarks(ROOT)
    old = gsb.remarks(Path(args.parent_src).resolve()) if args.parent_src else {}
    lines = ["kernels of cat_render.hip, hipcc -Rpass-analysis=kernel-resource-usage (gfx950)" + (": this tree / parent" if old else ""),
             f"  {'kernel':28s} {'SGPR':>9s} {'VGPR':>9s} {'scratch':>9s} {'occ':>7s}"]
    for name, a in new.items():
        b = old.get(name)
        cell = lambda k: f"{a[k]}/{b[k]}" if b else (f"{a[k]}/-" if old else str(a[k]))
        lines.append(f"  {name:28s} {cell('sgpr'):>9s} {cell('vgpr'):>9s} {cell('scratch'):>9s} {cell('occupancy'):>7s}")
    if old:
        changed = [n for n in old if new.get(n) != old[n]]
        lines.append("the other kernels keep their figures" if not changed else "CHANGED against the parent: " + ", ".join(changed))
    lines.append("nav_spawn_kernel: a wavefront per slot; the cells chosen so far live one per lane and come back through a lane read, the sweep's "
                 "predicate goes through a ballot and its count is scalar: hence few VGPRs; no scratch, no LDS")
    return lines


def fallback(args) -> list:
    import numpy as np
    import torch
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.navigation import NONE, NavField, spawn_step
    N = 4096
    lines = [f"navigation.spawn_step on the arena field, 2v1 x {N} slots, all masked, torch.rand draws (seed 1); share of slots the rule cannot place"]
    for name in ("squarinth", "labyrinth"):
        field = NavField.from_maps([load_preset(name, 2, 1).compile()], np.zeros(N, np.int32), 16, 6.0, "cpu", arena=True)
        free, hops = field.free_of(0), field.hops_of(0)
        idx = np.flatnonzero(free)
        sub = hops[np.ix_(idx, idx)]
        lines.append(f"  {name}: {len(idx)} free cells, diameter {int(sub[sub != NONE].max())}")
        for lo, hi in (BAND, (8, 12), (30, 34), (60, 64)):
            u = torch.rand(3, N, generator=torch.Generator().manual_seed(1))
            _, placed = spawn_step(torch.ones(N, dtype=torch.uint8), u, torch.tensor([[lo, hi]] * N, dtype=torch.int32), field, 2)
            cand = ((sub >= lo) & (sub <= hi)).sum(axis=1)
            lines.append(f"    band ({lo}, {hi}): fallback share {1.0 - float(placed.float().mean()):.4f}; candidates per anchor min {int(cand.min())}, "
                         f"anchors with none {int((cand == 0).sum())}")
    return lines


def launch(args) -> list:
    import torch
    from as_cops_and_thieves_amd import VecCopsEnv, _learn_native as ln, load_preset
    from as_cops_and_thieves_amd.selfplay.curriculum import GeodesicSpawner
    N, L = 4096, 200
    env = VecCopsEnv(load_preset("labyrinth", 2, 1), N, num_rays=64, max_step_count=400, seed=3)
    env.reset()
    for t in range(50):
        env.step_raw(env.random_actions(t))
    sp = GeodesicSpawner(env, *BAND)
    raw = {"terminated": (torch.rand(N, device="cuda") < 0.01).to(torch.uint8), "winner": torch.zeros(N, dtype=torch.int8, device="cuda")}
    u = torch.rand(3, N, device="cuda")
    fmt = lambda v: f"median {statistics.median(v):.2f} us, range {min(v):.2f} .. {max(v):.2f}"
    lines = [f"labyrinth 2v1 x {N}, band {BAND}, {int(raw['terminated'].sum())} slots masked; {torch.cuda.get_device_name(0)}; {L} calls per measurement, 7 measurements"]
    for what, fn in (("respawn (spawn kernel + counters + masked cat_reset)", lambda: sp.respawn(raw, u)),
                     ("cat_render_nav_spawn alone", lambda: ln.nav_spawn(raw["terminated"], u, sp.band, sp.field, sp.n_cops, sp.positions, sp.placed))):
        many = lambda: [fn() for _ in range(L)]
        many(); torch.cuda.synchronize()
        eager = [1e3 * ms / L for ms in gsb.timed(many, 7)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            many()
        graph.replay(); torch.cuda.synchronize()
        replay = [1e3 * ms / L for ms in gsb.timed(graph.replay, 7)]
        lines += [f"  {what}", f"    back to back (host-bound):          {fmt(eager)} per call", f"    replayed from one graph of {L} calls: {fmt(replay)} per call"]
    env.check_errors()
    env.close()
    return lines


def make_trainer(on: bool, N, horizon, seed=2, adapt=False, **tc):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    env = VecCopsEnv(load_preset("squarinth", 2, 1), N, num_rays=64, max_step_count=400, seed=5, track_episodes=True)
    rc = RoleConfig(random_timesteps=0, learning_starts=0)
    cur = dict(spawn_curriculum=BAND, **({"curriculum_adapt": ADAPT, "curriculum_max": HI_MAX} if adapt else {})) if on else {}
    cfg = TrainerConfig(horizon=horizon, policy_freeze_duration=0, opponent_freeze_duration=0, **cur, **tc)
    return env, MAPPOTrainer(env, {"cop": rc, "thief": rc}, cfg, seed=seed)


def trainer(args) -> list:
    import torch
    N, H, reps = 1024, 64, max(7, args.reps)
    legs = {"off": make_trainer(False, N, H), "on": make_trainer(True, N, H)}

    def leg(tr):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tr.collect(); tr.update()
        torch.cuda.synchronize()
        return N * H / (time.perf_counter() - t0)

    for _ in range(3):                                  # eager rollout, capture, first replay; the update's graph
        for _, tr in legs.values():
            leg(tr)
    got = {k: [] for k in legs}
    for r in range(reps):
        for k in (("off", "on") if r % 2 == 0 else ("on", "off")):
            got[k].append(leg(legs[k][1]))
    lines = [f"squarinth 2v1 x {N}, horizon {H}, bptt 16, band {BAND} on every slot; {torch.cuda.get_device_name(0)}; one process, legs alternating (order "
             f"reversed every other repetition), {reps} repetitions after 3 warm-up legs each; a leg = collect() + update() between two synchronisations",
             "  env-steps/s (N * horizon / wall time of the leg)"]
    for k, v in got.items():
        lines.append(f"  {k:3s} median {statistics.median(v):12.0f}  min {min(v):12.0f}  max {max(v):12.0f}   all: " + " ".join(f"{x:.0f}" for x in v))
    lines.append(f"  on median / off median = {statistics.median(got['on']) / statistics.median(got['off']):.4f}")
    lines.append(f"  on: {legs['on'][1]._spawner.counters()}")
    for env, _ in legs.values():
        env.close()
    return lines


def learning(args) -> list:
    N, H, U = 1024, 128, args.updates
    lines = [f"squarinth 2v1 x {N}, horizon {H}, max_step_count 400, thieves random (random_action_roles), {U} updates each, the same seed; then every "
             f"slot off (the map's own spawn) and the cops' win rate over the episodes finished during {U // 4} more rollouts without an update; ONE run each"]
    for name, on in (("off", False), ("on", True)):
        env, tr = make_trainer(on, N, H, adapt=True, random_action_roles=("thief",))
        for _ in range(U):
            tr.collect(); tr.update()
        during = env.episode_stats(clear=True)
        extra = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in tr.read_stats().items() if k.startswith("curriculum/")}
        if on:
            tr._spawner.set_off()
        tr.reset_episodes()
        env.episode_stats(clear=True)
        for _ in range(U // 4):
            tr.collect()
        e = env.episode_stats()
        lines.append(f"  {name:3s}: on the map's own spawn cop win rate {e['cop_win_rate']:.3f} over {e['episodes']} episodes, mean length {e['mean_length']:.1f}; "
                     f"while training {during['cop_win_rate']:.3f} over {during['episodes']} episodes  {extra}")
        env.close()
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=SECTIONS)
    ap.add_argument("--parent-src", type=Path, help="resources: a checkout of the parent commit to compare the other kernels with")
    ap.add_argument("--reps", type=int, default=7, help="trainer: repetitions per leg (at least 7)")
    ap.add_argument("--updates", type=int, default=150, help="learning: updates per run")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "curriculum.txt")
    args = ap.parse_args()
    if args.mode in ("launch", "trainer", "learning"):
        import torch
        if not torch.cuda.is_available():
            raise SystemExit(f"curriculum_bench {args.mode} needs a GPU")
    lines = globals()[args.mode](args)
    print("\n".join(lines), flush=True)
    gsb.SECTIONS = SECTIONS
    gsb.write_section(args.out, args.mode, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
