#!/usr/bin/env python3
"""Watch a checkpoint play: the headless counterpart of the reference's ``src/self_play_eval.py`` (which runs
``SimpleEnv(render_mode="human")`` on a checkpoint), on the batched env and the GPU frame renderer.

    python -m as_cops_and_thieves_amd.selfplay.watch --map agh-map --envs 4 --checkpoint run/joint_iter_3_full_agent.pt \\
        --ticks 2000 --rays --out clips/

K env slots play one episode each with the policies' sampled actions, as ``self_play.evaluate_agents`` plays them; a slot stops at
its first termination (capture or timeout).  Every tick the K envs are drawn in ONE launch (``VecCopsEnv.render``) and written as
``DIR/env_{k}/frame_{t:05d}.png`` -- frame 0 is the reset state, frame t the state after tick t, the last one the terminal tick --
and ``DIR/episode.json`` records each slot's winner and length.  Without ``--checkpoint`` the policies are freshly initialised.
The env does not reset finished episodes (``auto_reset=False``), so a slot's last frame shows how its episode ended.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, Optional

import torch

from ..environments import WINNER_NAMES, VecCopsEnv
from ..maps import load_preset
from ..render import write_png
from .mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
from .self_play import _initial_states, _skip_kw, _trainer_actions


def make_env(map_name: str, envs: int, seed: int = 0, num_rays: int = 64, max_step_count: int = 2000, n_cops: Optional[int] = None,
             n_thieves: Optional[int] = None, device=None, final_positions: bool = False) -> VecCopsEnv:
    """The env ``watch`` plays on (its reset state is what frame 0 shows)."""
    preset = load_preset(map_name, n_cops, n_thieves)
    return VecCopsEnv(preset, envs, num_rays=num_rays, max_step_count=max_step_count, seed=seed, device=device, auto_reset=False,
                      final_positions=final_positions)


@torch.no_grad()
def watch(map_name: str, envs: int, out_dir, checkpoint: Optional[str] = None, ticks: int = 2000, rays: bool = False, seed: int = 0,
          num_rays: int = 64, max_step_count: int = 2000, n_cops: Optional[int] = None, n_thieves: Optional[int] = None, device=None,
          log=print, fused_act: bool = False, greedy: bool = False, frame_skip: int = 1, heatmap: Optional[int] = None,
          scripts: Optional[Dict[str, str]] = None, navigators: Optional[Dict[str, str]] = None) -> Dict[str, object]:
    """``navigators``: {"cop": "pursue"} and / or {"thief": "flee"} -- that role's agents follow the PRIVILEGED navigator of
    ``navigators.py`` (it reads every agent's true position and the map, which no policy sees) instead of their policies; a role takes a
    script or a navigator, not both.
    ``scripts``: {"cop": "chase"} and / or {"thief": "evade"} -- that role's agents follow the scripted opponent of ``scripted.py``
    instead of their policies (their action columns are written over the policies' every tick).
    ``heatmap=CELL``: a ``positions.PositionTracker`` on a grid of CELL x CELL pixels is fed every decision's rows of the slots still
    playing (this env does not auto-reset, so the terminal row holds the episode's last position and counts as occupancy, and there is no
    spawn map), and ``heatmaps/`` next to the clips receives the pictures and ``positions.npz`` (``render.write_heatmaps``).  The env is
    built with ``final_positions=True``, so the capture / timeout maps of the episodes played are among them.
    ``frame_skip`` k > 1: the policies decide once per ``env.step(actions, repeat=k)`` and one frame is drawn per decision; ``ticks`` is then
    the most decisions played, a slot's ``length`` stays in env ticks (the sum of its ``infos["ticks"]``).
    ``fused_act``: no trainer is built -- a ``PolicyActor`` reads the checkpoint's policy blocks and acts (on a GPU: one launch per tick,
    ``include/cat_act.h``).  ``greedy`` (with ``fused_act``): the most probable action instead of a draw."""
    out_dir = Path(out_dir)
    skip = _skip_kw(frame_skip)
    torch.manual_seed(seed)
    env = make_env(map_name, envs, seed, num_rays, max_step_count, n_cops, n_thieves, device, final_positions=heatmap is not None)
    if greedy and not fused_act:
        raise ValueError("greedy=True needs fused_act=True (the default path samples, as self_play.evaluate_agents)")
    actor = None
    if fused_act:
        from .actor import PolicyActor
        actor, runner = PolicyActor.from_checkpoint(checkpoint, env, fused="kernel", seed=seed), None
    else:
        runner = MAPPOTrainer(env, {"cop": CFG_AGENT, "thief": CFG_AGENT}, TrainerConfig(graph_rollout=False, graph_update=False), seed=seed)
        if checkpoint:
            runner.load_state_dict(torch.load(checkpoint, map_location=runner.device, weights_only=True), optimizer=False)
    scripted = None
    if scripts:
        from .scripted import ScriptedActor
        if any(r not in ("cop", "thief") for r in scripts):
            raise ValueError(f"scripts names roles: cop and / or thief, not {sorted(scripts)}")
        scripted = ScriptedActor(env, {a: scripts[a.split("_")[0]] for a in env.possible_agents if a.split("_")[0] in scripts})
    navigator = None
    if navigators:
        from .navigators import NavigatorActor
        if any(r not in ("cop", "thief") for r in navigators) or any(r in (scripts or {}) for r in navigators):
            raise ValueError(f"navigators names roles (cop and / or thief) that follow no script, not {sorted(navigators)}")
        navigator = NavigatorActor(env, {a: navigators[a.split("_")[0]] for a in env.possible_agents if a.split("_")[0] in navigators})
    N = env.num_envs
    W, H = (int(v) for v in env.maps[0].window_dimensions)
    slots = list(range(N))
    dirs = [out_dir / f"env_{k}" for k in slots]
    for d in dirs:
        d.mkdir(parents=True, exist_ok=True)

    def save(t: int, open_host):
        frames = env.render(slots, rays=rays).cpu().numpy()          # one launch for the K envs, one copy to the host
        for k in slots:
            if open_host[k]:
                write_png(dirs[k] / f"frame_{t:05d}.png", frames[k, :W, :H])

    tracker = None
    if heatmap is not None:
        from ..positions import PositionTracker
        tracker = PositionTracker(N, env.possible_agents, len(env.cops), (W, H), heatmap, 1, env.device, final_positions=True)
        never = torch.zeros(N, dtype=torch.uint8, device=env.device)
    obs, _ = env.reset()
    who = actor if actor is not None else runner
    starts = torch.ones(N, dtype=torch.bool, device=who.device)
    state = _initial_states(runner, actor, N)
    actions = torch.zeros(N, len(who.agents), dtype=torch.int32, device=who.device)
    open_host = [True] * N
    winner, length, ended = [None] * N, [ticks] * N, [False] * N
    played = [0] * N                                                      # frame_skip > 1: env ticks of the slot's episode so far
    save(0, open_host)
    for t in range(1, ticks + 1):
        if actor is not None:
            actions = actor.act(env, starts, greedy=greedy, obs=obs)
        else:
            _trainer_actions(runner, obs, state, starts, actions, ())     # self_play.evaluate_agents' action selection
        if scripted is not None:
            scripted.act(env, starts, obs=obs, actions=actions)
        if navigator is not None:
            navigator.act(env, starts, actions=actions)
        obs, _, terms, _, infos = env.step(actions, **skip)
        starts = torch.zeros_like(starts)
        save(t, open_host)
        if tracker is not None:
            raw = env.raw_outputs()
            tracker.set_groups([0 if o else -1 for o in open_host])
            tracker.update(raw["team_positions"], never, raw["obs_type"])
            tracker.update_ends(raw["final_positions"], raw["terminated"], raw["truncated"])     # where the slots that ended just now did
        done = terms[who.agents[0]].cpu().tolist()
        win = infos["winner"].cpu().tolist()
        if skip:
            for k, n in enumerate(infos["ticks"].cpu().tolist()):
                if open_host[k]:
                    played[k] += n
                    length[k] = played[k]
        for k in slots:
            if open_host[k] and done[k]:
                open_host[k], ended[k], length[k], winner[k] = False, True, played[k] if skip else t, WINNER_NAMES[int(win[k])]
        if not any(open_host):
            break
    env.check_errors()
    frames_of = [(length[k] + 1) if ended[k] and not skip else (t + 1) for k in slots]
    result = {"map": map_name, "envs": N, "ticks": ticks, "checkpoint": checkpoint, "seed": seed, "rays": bool(rays),
              **({"fused_act": True, "greedy": bool(greedy)} if fused_act else {}), **({"frame_skip": frame_skip} if skip else {}),
              **({"scripts": dict(scripts)} if scripts else {}), **({"navigators": dict(navigators)} if navigators else {}),
              "slots": [{"env": k, "winner": winner[k], "length": length[k], "terminated": ended[k], "frames": frames_of[k]} for k in slots]}
    (out_dir / "episode.json").write_text(json.dumps(result, indent=1))
    if tracker is not None:
        from ..render import write_heatmaps
        write_heatmaps(out_dir / "heatmaps", tracker, env.maps)
    for s in result["slots"]:
        log(f"[watch] env {s['env']}: {'winner ' + str(s['winner']) if s['terminated'] else 'no termination'} after {s['length']} ticks")
    env.close()
    return result


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--map", default="squarinth")
    ap.add_argument("--envs", type=int, default=4, help="env slots K (one episode each, drawn in one launch per tick)")
    ap.add_argument("--checkpoint", default=None, help="a self-play checkpoint (joint_iter_*_full_agent.pt); fresh policies without it")
    ap.add_argument("--ticks", type=int, default=2000, help="ticks at most")
    ap.add_argument("--rays", action="store_true", help="draw every agent's ray fan, coloured by what each ray hit")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num-rays", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=2000, help="episode length limit of the env (the self-play driver's 2000)")
    ap.add_argument("--fused-act", action="store_true", help="act through a PolicyActor built straight from the checkpoint (no trainer; on a "
                    "GPU one launch per tick)")
    ap.add_argument("--greedy", action="store_true", help="with --fused-act: the most probable action instead of a draw")
    ap.add_argument("--frame-skip", type=int, default=1, help="env ticks per decision (action repeat); one frame per decision, --ticks counts decisions")
    ap.add_argument("--heatmap", type=int, default=None, metavar="CELL", help="also write occupancy / exposure heatmaps of the episodes played, on a "
                    "grid of CELL x CELL pixels, into heatmaps/ next to the clips")
    ap.add_argument("--script", action="append", default=[], metavar="ROLE=NAME", help="cop=chase or thief=evade: that role follows the scripted "
                    "opponent instead of its policy (may be given once per role)")
    ap.add_argument("--navigator", action="append", default=[], metavar="ROLE=NAME", help="cop=pursue or thief=flee: that role follows the PRIVILEGED "
                    "shortest-path navigator (it reads true positions and the map) instead of its policy (may be given once per role)")
    args = ap.parse_args(argv)
    navigators = {}
    for item in args.navigator:
        role, _, name = item.partition("=")
        if (role, name) not in (("cop", "pursue"), ("thief", "flee")):
            ap.error(f"--navigator takes cop=pursue or thief=flee, not {item!r}")
        navigators[role] = name
    scripts = {}
    for item in args.script:
        role, _, name = item.partition("=")
        if role not in ("cop", "thief") or name not in ("chase", "evade"):
            ap.error(f"--script takes cop=chase, cop=evade, thief=chase or thief=evade, not {item!r}")
        scripts[role] = name
    if set(scripts) & set(navigators):
        ap.error("a role follows a --script or a --navigator, not both")
    if args.heatmap is not None and args.heatmap < 1:
        ap.error("--heatmap must be >= 1")
    if args.envs < 1 or args.ticks < 1 or args.frame_skip < 1:
        ap.error("--envs, --ticks and --frame-skip must be >= 1")
    if args.greedy and not args.fused_act:
        ap.error("--greedy needs --fused-act")
    watch(args.map, args.envs, args.out, args.checkpoint, args.ticks, args.rays, args.seed, args.num_rays, args.max_steps,
          fused_act=args.fused_act, greedy=args.greedy, frame_skip=args.frame_skip, heatmap=args.heatmap, scripts=scripts or None, navigators=navigators or None)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
