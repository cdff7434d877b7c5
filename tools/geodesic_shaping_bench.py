#!/usr/bin/env python3
"""What geodesic reward shaping (``TrainerConfig.geodesic_shaping``, ``cat_render_nav_shape``) costs and does.  Each mode rewrites its own
section of the output file (default profiles/geodesic_shaping.txt) and keeps the others.  No threshold anywhere: the figures are written
down as measured.

    python tools/geodesic_shaping_bench.py resources [--parent-src PARENT]     # no GPU: registers of the kernels of cat_render.hip
    python tools/geodesic_shaping_bench.py share                               # no GPU: episodes with every separation defined (oracle env)
    python tools/geodesic_shaping_bench.py launch                              # GPU: per-launch time, back to back and from a graph
    python tools/geodesic_shaping_bench.py trainer [--reps 7]                  # GPU: collect + update rate, option off / on
    python tools/geodesic_shaping_bench.py learning [--updates 150]            # GPU: cops against random thieves on squarinth, off / on

``resources``: ``-Rpass-analysis=kernel-resource-usage`` of cat_render.hip; with ``--parent-src`` (a checkout of the parent commit) the
other kernels' figures stand beside the parent's.
``share``: squarinth 2v1 x 256 on the oracle-backed stand-in env, cops "pursue", thieves random, 200 ticks: the share of completed episode
rows whose separations were all defined, on the navigators' plain field and on the arena field the shaper builds.
``launch``: labyrinth 2v1 x 4096, G = 3: 200 launches back to back between two events, and a graph of 200 launches replayed, 7 times each.
``trainer``: squarinth 2v1 x 1024, horizon 64: one process, two trainers (off, on), legs alternating, each leg one collect() + update()
between two synchronisations; medians and ranges of ``--reps`` repetitions and the ratio to the OFF leg of the same run.
``learning``: squarinth 2v1 x 1024, horizon 128, thieves random (``random_action_roles``), ``--updates`` updates each, the same seed: the
cops' win rate over the episodes of the last quarter of the updates, off and on.  One run each: a figure, not a finding.
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SECTIONS = ("resources", "share", "launch", "trainer", "learning")


def remarks(src_root: Path) -> dict:
    """kernel name -> {sgpr, vgpr, scratch, occupancy} of cat_render.hip under ``src_root``."""
    from as_cops_and_thieves_amd import _learn_native as ln
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = src_root / "as_cops_and_thieves_amd" / "csrc"
    res = subprocess.run([hipcc, *ln.HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", f"-I{src_root / 'include'}", f"-I{src}", "-o", os.devnull,
                          str(src / "cat_render.hip")], capture_output=True, text=True)
    if res.returncode != 0:
        raise SystemExit(f"hipcc failed on {src_root}:\n{res.stderr[-2000:]}")
    fields = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}
    table, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: \S*?\d+([a-z_]+_kernel)E", line)
        if m:
            name = m.group(1)
            table[name] = {}
        for label, key in fields.items():
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and name is not None:
                table[name][key] = int(m.group(1))
    return table


def resources(args) -> list:
    new = remarks(ROOT)
    old = remarks(Path(args.parent_src).resolve()) if args.parent_src else {}
    lines = ["kernels of cat_render.hip, hipcc -Rpass-analysis=kernel-resource-usage (gfx950)" + (": this tree / parent" if old else ""),
             f"  {'kernel':28s} {'SGPR':>9s} {'VGPR':>9s} {'scratch':>9s} {'occ':>7s}"]
    for name, a in new.items():
        b = old.get(name)
        cell = lambda k: f"{a[k]}/{b[k]}" if b else (f"{a[k]}/-" if old else str(a[k]))
        lines.append(f"  {name:28s} {cell('sgpr'):>9s} {cell('vgpr'):>9s} {cell('scratch'):>9s} {cell('occupancy'):>7s}")
    if old:
        changed = [n for n in old if new.get(n) != old[n]]
        lines.append("the other kernels keep their figures" if not changed else "CHANGED against the parent: " + ", ".join(changed))
    lines.append("nav_shape_kernel: a thread per slot; the cells of up to 16 agents of team_positions and of final_positions stay in registers "
                 "(the loops over agents are unrolled so that no register array is indexed by a variable), hence the VGPR count; no scratch, no LDS")
    return lines


def share(args) -> list:
    import torch
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.navigation import NavField, separation
    from as_cops_and_thieves_amd.selfplay.navigators import NavigatorActor
    from tests.shaping_env import ShapingOracleEnv
    N, T = 256, 200
    lines = [f"squarinth 2v1 x {N} on the oracle-backed stand-in env, cops pursue, thieves random, {T} ticks, max_step_count 400; a row = (agent, episode)"]
    for arena in (False, True):
        env = ShapingOracleEnv(load_preset("squarinth", 2, 1).compile(), N, num_rays=64, max_step_count=400, seed=7)
        env.reset()
        field = NavField.from_env(env, arena=arena)
        actor = NavigatorActor(env, {"cop_0": "pursue", "cop_1": "pursue"})
        gen = torch.Generator().manual_seed(1)
        agents, opp = [0, 1, 2], [0b100, 0b100, 0b011]
        ok = separation(env.raw_outputs()["team_positions"], field, agents, opp) >= 0
        done = good = captures = 0
        for _ in range(T):
            acts = torch.randint(0, 4, (N, 3), generator=gen, dtype=torch.int32)
            actor.act(env, actions=acts)
            env.step(acts)
            raw = env.raw_outputs()
            term, trunc = raw["terminated"].bool(), raw["truncated"].bool()
            now = separation(raw["team_positions"], field, agents, opp) >= 0
            fin = separation(raw["final_positions"], field, agents, opp) >= 0
            ok &= torch.where(term & ~trunc, torch.ones_like(ok), torch.where(term, fin, now))
            done += 3 * int(term.sum()); good += int(ok[:, term].sum()); captures += int((term & ~trunc).sum())
            ok = torch.where(term, now, ok)
        lines.append(f"  {'arena field (the shaper default)' if arena else 'plain field (the navigators)  '}: free-cell components {field.component_sizes()[0]}, "
                     f"{captures} captures, completed rows {done}, every separation defined {good}: share {good / max(done, 1):.3f}")
    return lines


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def launch(args) -> list:
    import torch
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.shaping import GeodesicShaper
    N, L = 4096, 200
    env = VecCopsEnv(load_preset("labyrinth", 2, 1), N, num_rays=64, max_step_count=400, seed=3, final_positions=True)
    env.reset()
    for t in range(50):
        raw = env.step_raw(env.random_actions(t))
    sh = GeodesicShaper(env, env.possible_agents, scale_cop=0.05, scale_thief=0.05, gamma=0.99)
    rew, shp = torch.zeros(3, N, device="cuda"), torch.zeros(3, N, device="cuda")
    sh.prime(raw)
    many = lambda: [sh.step(raw, rew, shp) for _ in range(L)]
    many(); torch.cuda.synchronize()
    eager = [1e3 * ms / L for ms in timed(many, 7)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        many()
    graph.replay(); torch.cuda.synchronize()
    replay = [1e3 * ms / L for ms in timed(graph.replay, 7)]
    env.close()
    fmt = lambda v: f"median {statistics.median(v):.2f} us, range {min(v):.2f} .. {max(v):.2f}"
    return [f"labyrinth 2v1 x {N}, G = 3; {torch.cuda.get_device_name(0)}; {L} launches of cat_render_nav_shape per measurement, 7 measurements",
            f"  back to back (host-bound: ctypes call per launch): {fmt(eager)} per launch",
            f"  replayed from one graph of {L} launches:          {fmt(replay)} per launch"]


def make_trainer(shaping, N, horizon, seed=2, **tc):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    env = VecCopsEnv(load_preset("squarinth", 2, 1), N, num_rays=64, max_step_count=400, seed=5, final_positions=True, track_episodes=True)
    rc = RoleConfig(random_timesteps=0, learning_starts=0)
    cfg = TrainerConfig(horizon=horizon, policy_freeze_duration=0, opponent_freeze_duration=0, **({"geodesic_shaping": shaping} if shaping else {}), **tc)
    return env, MAPPOTrainer(env, {"cop": rc, "thief": rc}, cfg, seed=seed)


def trainer(args) -> list:
    import torch
    N, H, reps = 1024, 64, max(7, args.reps)
    legs = {"off": make_trainer(0.0, N, H), "on": make_trainer(0.05, N, H)}

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
    lines = [f"squarinth 2v1 x {N}, horizon {H}, bptt 16; {torch.cuda.get_device_name(0)}; one process, legs alternating (order reversed every other "
             f"repetition), {reps} repetitions after 3 warm-up legs each; a leg = collect() + update() between two synchronisations",
             "  env-steps/s (N * horizon / wall time of the leg)"]
    for k, v in got.items():
        lines.append(f"  {k:3s} median {statistics.median(v):12.0f}  min {min(v):12.0f}  max {max(v):12.0f}   all: " + " ".join(f"{x:.0f}" for x in v))
    lines.append(f"  on median / off median = {statistics.median(got['on']) / statistics.median(got['off']):.4f}")
    for env, _ in legs.values():
        env.close()
    return lines


def learning(args) -> list:
    import torch
    N, H, U = 1024, 128, args.updates
    lines = [f"squarinth 2v1 x {N}, horizon {H}, max_step_count 400, thieves random (random_action_roles), {U} updates each, the same seed; "
             f"cops' win rate over the episodes finished during the last {U // 4} updates; ONE run each"]
    for name, w in (("off", 0.0), ("on", args.scale)):
        env, tr = make_trainer(w, N, H, random_action_roles=("thief",), **({"shaping_scale_thief": 0.0} if w else {}))
        for u in range(U):
            if u == U - U // 4:
                env.episode_stats(clear=True)
            tr.collect(); tr.update()
        e = env.episode_stats()
        extra = {k: round(v, 4) for k, v in tr.read_stats().items() if k.startswith(("shaping/", "geodesic_hops/"))}
        lines.append(f"  {name:3s} (geodesic_shaping {w}): cop win rate {e['cop_win_rate']:.3f} over {e['episodes']} episodes, mean length {e['mean_length']:.1f}  {extra}")
        env.close()
    return lines


def write_section(out: Path, section: str, lines: list) -> None:
    """Replace ``[section]`` of the file (up to the next ``[...]`` header or the end), keep everything else, in the order of SECTIONS."""
    text = out.read_text() if out.exists() else ""
    parts = [p for p in re.split(r"(?m)^(?=\[[a-z]+\]$)", text) if p.strip() and not p.startswith(f"[{section}]")]
    parts.append(f"[{section}]\n" + "\n".join(lines) + "\n\n")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(sorted(parts, key=lambda p: next((i for i, s in enumerate(SECTIONS) if p.startswith(f"[{s}]")), -1))))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=SECTIONS)
    ap.add_argument("--parent-src", type=Path, help="resources: a checkout of the parent commit to compare the other kernels with")
    ap.add_argument("--reps", type=int, default=7, help="trainer: repetitions per leg (at least 7)")
    ap.add_argument("--updates", type=int, default=150, help="learning: updates per run")
    ap.add_argument("--scale", type=float, default=0.05, help="learning: the cops' geodesic_shaping")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "geodesic_shaping.txt")
    args = ap.parse_args()
    if args.mode in ("launch", "trainer", "learning"):
        import torch
        if not torch.cuda.is_available():
            raise SystemExit(f"geodesic_shaping_bench {args.mode} needs a GPU")
    lines = globals()[args.mode](args)
    print("\n".join(lines), flush=True)
    write_section(args.out, args.mode, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
