#!/usr/bin/env python3
"""Cross-play: every archived cop policy against every archived thief policy, many cells of the table per pass.

    python -m as_cops_and_thieves_amd.selfplay.crossplay --cops run/cops --thieves run/thieves --map squarinth --episodes 32 --out payoff.json

A cell (cop file i, thief file j) is one segment of ``--episodes`` env slots of a ``LeagueActor`` (``actor.py``): the cops of file i and
the thieves of file j play the first episode of each slot (``self_play.evaluate_league``).  At most ``ACT_MAX_SEGMENTS`` = 32 cells share a
pass, so a K x K table takes ceil(K^2 / 32) passes instead of K^2.  ``--random-column`` adds a last column: thieves acting uniformly at
random, a fixed yardstick; ``--scripted`` adds the scripted opponents of ``scripted.py``: a last row ``chase`` (cops that head for the
thief they see) and a last column ``evade`` (thieves that run from the cops they see).  ``payoff.json`` holds the file lists and the
matrices ``cop_win_rate``, ``cop_wins``, ``thief_wins``, ``timeouts`` (the three counts add up to the episodes of a cell) and
``mean_length`` (ticks of the counted episodes), rows = cop files.
``--heatmaps DIR [--cell C]``: position statistics of the counted episodes, one group per cell of the table -- occupancy, exposure, hidden
and spawn maps per agent under ``DIR/{cop file}__{thief file}/`` and the raw counts in ``DIR/positions.npz`` (``positions.py``).
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, List, Optional, Union

import torch

from .. import _learn_native
from . import archive
from .actor import LeagueActor
from .self_play import evaluate_league

RANDOM = "random"
CHASE, EVADE = "chase", "evade"                 # scripted.SCRIPTS: the row of scripted cops, the column of scripted thieves


def policy_files(directory, role: str) -> List[Path]:
    """The archive's ``{role}_iter_N.pt`` files in iteration order; a directory without any: every ``*.pt`` in it by name."""
    files = archive._policy_files(Path(directory), role)
    return files or sorted(Path(directory).glob("*.pt"))


@torch.no_grad()
def crossplay(cops, thieves, map_name: str, episodes: int, random_column: bool = False, greedy: bool = False, num_rays: int = 64,
              n_cops: Optional[int] = None, n_thieves: Optional[int] = None, max_step_count: int = 2000, seed: int = 0, device=None,
              fused: Union[str, bool] = "kernel", normalize_inputs: bool = False, env_factory=None, log=None,
              frame_skip: int = 1, heatmaps=None, cell: int = 8, scripted: bool = False) -> Dict[str, object]:
    """``cops`` / ``thieves``: an archive directory or a list of checkpoint files.  ``episodes`` slots per cell; sampled actions, or the
    largest logit with ``greedy``.  ``scripted``: a last row of "chase" cops and a last column of "evade" thieves (after "random").
    ``env_factory(num_envs, seed)``: build the env some other way (``map_name`` etc. are then unused).
    ``frame_skip``: env ticks per decision (``evaluate_league``); ``mean_length`` stays in env ticks.
    ``heatmaps``: a directory -- the env is built with ``track_positions=cell`` and one group per cell of a pass, and every pass writes its
    cells' heatmaps there (``render.write_heatmaps``; ``positions.npz`` holds the first pass, ``positions_pass{p}.npz`` the later ones).  An
    ``env_factory``'s env must then bring a ``position_tracker`` of at least as many groups as a pass has segments.
    The sampled actions draw from torch's global generator: seed it for a reproducible table.  Returns what the module's docstring lists."""
    cop_files = [Path(f) for f in (cops if isinstance(cops, (list, tuple)) else policy_files(cops, "cop"))]
    thief_files = [Path(f) for f in (thieves if isinstance(thieves, (list, tuple)) else policy_files(thieves, "thief"))]
    if not cop_files or not thief_files:
        raise ValueError(f"cross-play needs at least one file per role: {len(cop_files)} cop and {len(thief_files)} thief files")
    if episodes < 1:
        raise ValueError("episodes must be at least 1")
    rows = list(range(len(cop_files))) + ([CHASE] if scripted else [])
    columns = list(range(len(thief_files))) + ([RANDOM] if random_column else []) + ([EVADE] if scripted else [])
    cells = [(i, j) for i in rows for j in columns]
    per_pass = min(_learn_native.ACT_MAX_SEGMENTS, len(cells))
    N = per_pass * episodes
    if env_factory is None:
        from ..environments import VecCopsEnv
        from ..maps import load_preset
        track = {} if heatmaps is None else {"track_positions": int(cell), "position_groups": per_pass, "final_positions": True}
        env = VecCopsEnv(load_preset(map_name, n_cops, n_thieves), N, num_rays=num_rays, max_step_count=max_step_count, seed=seed, device=device,
                         **track)
    else:
        env = env_factory(N, seed)
    agents = list(env.possible_agents)
    actor = LeagueActor.from_env(env, per_pass * len(agents), fused=fused, normalize_inputs=normalize_inputs, seed=seed, device=device)

    class _Greedy:                                      # evaluate_league's actor surface with greedy actions
        def __getattr__(self, name):
            return getattr(actor, name)

        def act(self, env_, starts=None, obs=None):
            return actor.act(env_, starts, greedy=True, obs=obs)
    player = _Greedy() if greedy else actor
    shape = (len(rows), len(columns))
    mats = {k: [[0] * shape[1] for _ in range(shape[0])] for k in ("cop_wins", "thief_wins", "timeouts")}
    mean_length = [[0.0] * shape[1] for _ in range(shape[0])]
    loaded: Dict[Path, dict] = {}
    passes = 0
    for p0 in range(0, len(cells), per_pass):
        chunk = cells[p0:p0 + per_pass]
        sets, segments, quota = {}, [], []

        def set_of(path: Path, agent: str) -> int:
            if (path, agent) not in sets:
                if path not in loaded:
                    loaded[path] = torch.load(path, map_location="cpu", weights_only=True)
                sets[(path, agent)] = len(sets)
                actor.load_set(sets[(path, agent)], loaded[path], agent)
            return sets[(path, agent)]
        for s, (i, j) in enumerate(chunk):
            who = {a: ((i if i == CHASE else set_of(cop_files[i], a)) if a.startswith("cop") else j if j in (RANDOM, EVADE) else set_of(thief_files[j], a))
                   for a in agents}
            segments.append((s * episodes, (s + 1) * episodes, who))
            quota.append(episodes)
        if len(chunk) < per_pass:                       # the last pass: the remaining slots fill the env and count nothing
            segments.append((len(chunk) * episodes, N, {a: RANDOM for a in agents}))
            quota.append(0)
        loaded.clear()
        actor.set_matchups(segments)
        res = evaluate_league(env, player, quota, frame_skip=frame_skip, **({} if heatmaps is None else {"positions": True}))
        if heatmaps is not None:
            from ..render import write_heatmaps
            tracker = env.position_tracker
            names = [f"{i if i == CHASE else cop_files[i].stem}__{j if j in (RANDOM, EVADE) else thief_files[j].stem}" for i, j in chunk]
            write_heatmaps(heatmaps, tracker, env.maps, group_names=names + [None] * (tracker.G - len(names)),
                           npz_name="positions.npz" if passes == 0 else f"positions_pass{passes}.npz")
        length = res["length"].cpu()
        for s, (i, j) in enumerate(chunk):
            row, col = rows.index(i), columns.index(j)
            for k in mats:
                mats[k][row][col] = res[k][s]
            mean_length[row][col] = float(length[s * episodes:(s + 1) * episodes].float().mean())
        passes += 1
        if log:
            log(f"[cross-play] pass {passes}: {len(chunk)} cells, {res['ticks']} ticks")
    env.close()
    return {"cops": [f.name for f in cop_files] + ([CHASE] if scripted else []),
            "thieves": [f.name for f in thief_files] + ([RANDOM] if random_column else []) + ([EVADE] if scripted else []),
            "episodes": episodes, "greedy": bool(greedy), "passes": passes,
            "cop_win_rate": [[w / episodes for w in row] for row in mats["cop_wins"]], **mats, "mean_length": mean_length}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cops", type=Path, required=True, help="archive directory of cop checkpoints")
    ap.add_argument("--thieves", type=Path, required=True, help="archive directory of thief checkpoints")
    ap.add_argument("--map", default="squarinth")
    ap.add_argument("--episodes", type=int, default=32, help="env slots (first episodes) per cell")
    ap.add_argument("--random-column", action="store_true", help="a last column of thieves acting uniformly at random")
    ap.add_argument("--scripted", action="store_true", help="a last row of scripted \"chase\" cops and a last column of scripted \"evade\" thieves")
    ap.add_argument("--greedy", action="store_true", help="the largest logit instead of a draw")
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--n-cops", type=int, default=None)
    ap.add_argument("--n-thieves", type=int, default=None)
    ap.add_argument("--max-step-count", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--frame-skip", type=int, default=1, help="env ticks per decision (action repeat)")
    ap.add_argument("--heatmaps", type=Path, default=None, metavar="DIR", help="write per-cell occupancy / exposure / spawn heatmaps and positions.npz there")
    ap.add_argument("--cell", type=int, default=8, help="with --heatmaps: the grid's cell size in pixels")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    res = crossplay(args.cops, args.thieves, args.map, args.episodes, args.random_column, args.greedy, args.rays, args.n_cops, args.n_thieves,
                    args.max_step_count, args.seed, log=print, frame_skip=args.frame_skip, heatmaps=args.heatmaps, cell=args.cell, scripted=args.scripted)
    args.out.write_text(json.dumps(res, indent=1))
    print(f"[cross-play] {len(res['cops'])} x {len(res['thieves'])} cells in {res['passes']} pass(es) -> {args.out}")


if __name__ == "__main__":
    main()
