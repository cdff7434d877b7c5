"""Navigator opponents: the strong fixed reference the scripted ``"chase"`` / ``"evade"`` are not -- a cop that takes the shortest path
around the walls to the nearest thief (``"pursue"``), a thief that moves to the neighbouring cell farthest, by shortest path, from the
nearest cop (``"flee"``).  Map-aware, parameter-free, deterministic but for the fallback draw.

PRIVILEGED: both decide from ``team_positions`` -- every agent's true position -- and the map's hop table (``navigation.NavField``),
neither of which a policy observes.  They are yardsticks that say how far a role is from one that knows the maze, never a fair opponent.

    actor = NavigatorActor(env, {"thief_0": "flee"})            # the thieves of a 2v1 env
    trainer.set_opponent("thief", actor)                        # the cops train against it; the rollout stays one captured graph
    actions = actor.act(env)                                    # or on its own: writes its agents' columns of [N, A]

``navigation.navigate_step`` IS the rule (torch, any device); on a GPU ``NavigatorActor`` runs it as one launch of ``cat_render_nav_step``
(include/cat_render.h), which equals it exactly.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _learn_native
from ..navigation import NavField, navigate_step

NAVIGATORS = {"pursue": 0, "flee": 1}
ROLE_OF = {"pursue": "cop", "flee": "thief"}


def navigator_code(name, agent: Optional[str] = None) -> int:
    """"pursue" / "flee" -> the kernel's code; None -> -1 (leaves the column alone there).  With ``agent``: "pursue" is for cops only and
    "flee" for thieves only.  ValueError otherwise."""
    if name is None:
        return -1
    if not (isinstance(name, str) and name in NAVIGATORS):
        raise ValueError(f"{name!r} is not a navigator: {sorted(NAVIGATORS)} or None")
    if agent is not None and not agent.startswith(ROLE_OF[name]):
        raise ValueError(f"{name!r} is a {ROLE_OF[name]}'s navigator: {agent} cannot follow it")
    return NAVIGATORS[name]


class NavigatorActor:
    """Navigator agents over ``env`` with the opponent surface ``MAPPOTrainer.set_opponent`` duck-types (``agents``, ``env_agents``, ``N``,
    ``device``, ``fused``, ``table``, ``actions``, ``segments``, ``reset``, ``get_state`` / ``set_state``, ``act``), as ``ScriptedActor``.

    ``navigators``: {agent: "pursue" | "flee"} for every agent the actor plays everywhere (one segment); ``agents``: the agents it covers,
    in the env's order (default: the keys of ``navigators``) -- ``set_segments`` then says per row range who follows what, None leaving an
    agent's column alone there.  ``field``: a ``NavField`` of the env to share (else ``NavField.from_env(env, cell)``).  An agent's
    opponents are all agents of the other team.

    ``fused`` is True on a GPU: per tick one ``torch.rand(G, N)`` and ONE launch of ``cat_render_nav_step``, capturable.  Elsewhere
    ``navigate_step``, from the same single ``torch.rand(G, N)``.  Both read ``env.raw_outputs()["team_positions"]``.  The rule has no
    state: ``reset`` / ``set_state`` do nothing and the state is an empty tensor.  ``nav_hops`` int32 [G, N] holds the last tick's hop count
    of every row to its target (-1 after the fallback): the geodesic separation."""

    def __init__(self, env, navigators: Optional[Dict[str, Optional[str]]] = None, agents: Optional[Sequence[str]] = None,
                 field: Optional[NavField] = None, cell: int = 16):
        self.device = torch.device(getattr(env, "device", "cpu"))
        self.env_agents = list(env.possible_agents)
        navigators = dict(navigators or {})
        chosen = list(navigators) if agents is None else list(agents)
        if not chosen or len(set(chosen)) != len(chosen) or any(a not in self.env_agents for a in chosen):
            raise ValueError(f"agents must be a non-empty subset of the env's agents {self.env_agents} without repeats: {chosen}")
        if any(a not in chosen for a in navigators):
            raise ValueError(f"navigators name agents the actor does not cover: {sorted(set(navigators) - set(chosen))}")
        self.agents: List[str] = [a for a in self.env_agents if a in chosen]
        if len(self.agents) > _learn_native.NAV_MAX_NAVIGATORS:
            raise ValueError(f"at most {_learn_native.NAV_MAX_NAVIGATORS} navigator agents")
        if len(self.env_agents) > _learn_native.RENDER_MAX_AGENTS:
            raise ValueError(f"at most {_learn_native.RENDER_MAX_AGENTS} agents per env")
        if not hasattr(env, "raw_outputs"):
            raise ValueError("a NavigatorActor reads the env core's team_positions buffer: the env must offer raw_outputs()")
        self.indices = [self.env_agents.index(a) for a in self.agents]
        cop = lambda a: a.startswith("cop")
        self.opponent_masks = [sum(1 << j for j, b in enumerate(self.env_agents) if cop(b) != cop(a)) for a in self.agents]
        self.N = env.num_envs
        self.G = len(self.agents)
        self.field = field if field is not None else NavField.from_env(env, cell)
        if self.field.device != self.device or tuple(self.field.slot_map.shape) != (self.N,):
            raise ValueError(f"the field must lie on {self.device} with a slot_map of {self.N} slots")
        self.fused = self.device.type == "cuda"
        self.actions = torch.zeros(self.N, len(self.env_agents), dtype=torch.int32, device=self.device)
        self.nav_hops = torch.full((self.G, self.N), -1, dtype=torch.int32, device=self.device)
        self.state = torch.empty(0, dtype=torch.int32, device=self.device)
        self._index_t = torch.tensor(self.indices, dtype=torch.long, device=self.device)
        self.table = None
        self.set_segments([(0, self.N, {a: navigators.get(a) for a in self.agents})])

    def set_segments(self, segments) -> None:
        """``segments``: [(start, stop, {agent: "pursue" | "flee" | None}), ...] -- contiguous row ranges that cover 0 .. N in order, every
        agent of the actor named in each.  ValueError otherwise (the current table then stays).  A new table is a new ``table`` object: a
        trainer that captured a rollout with the old one recaptures."""
        segments = list(segments)
        if not segments:
            raise ValueError("no segments")
        bounds = [segments[0][0]]
        rows = [[] for _ in self.agents]
        for lo, hi, who in segments:
            if lo != bounds[-1]:
                raise ValueError(f"segment ({lo}, {hi}) does not begin where the one before it ends ({bounds[-1]})")
            bounds.append(hi)
            if set(who) != set(self.agents):
                raise ValueError(f"segment ({lo}, {hi}) must name exactly the agents {self.agents}: {sorted(who)}")
            for g, a in enumerate(self.agents):
                rows[g].append(navigator_code(who[a], a))
        table = _learn_native.nav_table(self.N, self.G, bounds, rows)
        script = torch.empty(self.G, self.N, dtype=torch.int64)
        for s, (lo, hi) in enumerate(zip(table.start[:-1], table.start[1:])):
            for g in range(self.G):
                script[g, lo:hi] = table.rows[g][s]
        self.table, self._script_t = table, script.to(self.device)
        self.nav_hops.fill_(-1)                    # rows of a None segment are never written: they read -1

    @property
    def segments(self) -> List[Tuple[int, int]]:
        """[(start, stop)] of the current table."""
        b = self.table.start
        return list(zip(b[:-1], b[1:]))

    # ------------------------------------------------------------------ state: there is none
    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        pass

    def get_state(self, out=None):
        return self.state.clone() if out is None else out

    def set_state(self, state) -> None:
        pass

    # ------------------------------------------------------------------ the act tick
    @torch.no_grad()
    def act(self, env, starts: Optional[torch.Tensor] = None, obs=None, actions: Optional[torch.Tensor] = None, uniform=None) -> torch.Tensor:
        """The navigators' actions for the env's current positions, into their columns of ``actions`` (int32 [N, A] over ALL the env's
        agents; default ``self.actions``), which is returned; no other column is touched.  ``starts`` and ``obs`` are accepted for the
        opponent surface and not read.  ``uniform`` fp32 [G, N]: the tick's numbers instead of a fresh ``torch.rand(G, N)``."""
        if actions is None:
            actions = self.actions
        elif not (actions.dtype == torch.int32 and tuple(actions.shape) == tuple(self.actions.shape) and actions.is_contiguous()
                  and actions.device == self.actions.device):
            raise ValueError(f"actions must be a contiguous int32 {tuple(self.actions.shape)} tensor on {self.actions.device}")
        u = torch.rand(self.G, self.N, device=self.device) if uniform is None else uniform
        tp = env.raw_outputs()["team_positions"]
        if self.fused:
            _learn_native.nav_step(tp, u, self.field, self.indices, self.opponent_masks, self.table, actions, self.nav_hops)
            return actions
        act, hops = navigate_step(tp.to(self.device), u, self.field, self.indices, self._script_t, self.opponent_masks)
        self.nav_hops.copy_(hops)
        cols = actions.index_select(1, self._index_t)
        actions.index_copy_(1, self._index_t, torch.where(act.t() >= 0, act.t(), cols))
        return actions
