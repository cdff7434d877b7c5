"""Geodesic potential-based reward shaping (Ng, Harada and Russell 1999) for the learners of a rollout: ``F = gamma Phi(s') - Phi(s)`` with
``Phi`` a multiple of the shortest-path hop count to the nearest opponent (``navigation.NavField``), added to the LEARNER's reward rows.
The env's own ``reward``, its episode statistics and every observation stay as they are.  PRIVILEGED information (every agent's true
position and the map) reaches the learner through its reward only, never through an observation.

    shaper = GeodesicShaper(env, ["cop_0", "cop_1"], scale_cop=0.05, scale_thief=0.05, gamma=0.99)
    shaper.prime(env.raw_outputs())                          # the separations of the current state: before the first tick of a rollout
    raw = env.step_raw(actions)
    shaper.step(raw, rew[:, t], shape[:, t])                 # rew[g] += F, shape[g] = F; one launch on a GPU

``navigation.shaping_step`` IS the rule (torch, any device); on a GPU ``prime`` and ``step`` are one launch of ``cat_render_nav_shape``
(include/cat_render.h) each, which equals it bit for bit and is capturable.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from .. import _learn_native
from ..navigation import NavField, shaping_step

CAP_MAX = 65534


class GeodesicShaper:
    """The shaping state of ``agents`` (env agent names; kept in the env's order, without those whose scale is 0) over ``env``:
    ``hops_prev`` int32 [G, N], each row's geodesic separation from its nearest opponent at the start of the next tick (-1: undefined).

    ``scale_cop`` / ``scale_thief`` >= 0: the potential of a cop is ``-scale_cop * min(hops, cap)`` (closer is better), of a thief
    ``+scale_thief * min(hops, cap)``; an agent whose scale is 0 is left out (``agents`` then lacks it, and with nobody left ``G`` is 0 and
    ``prime`` / ``step`` do nothing).  ``gamma``: the learner's discount factor.  ``field``: a ``NavField`` of the env to share (else
    ``NavField.from_env(env, arena=True)``: the cells the map lets an agent reach, so that an agent in contact with a thin wall snaps to
    its own side of it -- with the navigators' plain field 42 % of squarinth's episodes lose a separation, profiles/geodesic_shaping.txt).  An agent's opponents are all agents of the other team.  ValueError names what is missing."""

    def __init__(self, env, agents: Sequence[str], *, scale_cop: float, scale_thief: float, cap: int = 64, gamma: float,
                 field: Optional[NavField] = None):
        self.device = torch.device(getattr(env, "device", "cpu"))
        self.env_agents: List[str] = list(env.possible_agents)
        for name, v in (("scale_cop", scale_cop), ("scale_thief", scale_thief)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma) or gamma < 0:
            raise ValueError(f"gamma must be a finite number >= 0, got {gamma!r}")
        if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap <= CAP_MAX:
            raise ValueError(f"cap is a hop count in 1 .. {CAP_MAX}, got {cap!r}")
        chosen = list(agents)
        if len(set(chosen)) != len(chosen) or any(a not in self.env_agents for a in chosen):
            raise ValueError(f"agents must be a subset of the env's agents {self.env_agents} without repeats: {chosen}")
        if not hasattr(env, "raw_outputs"):
            raise ValueError("a GeodesicShaper reads the env core's position buffers: the env must offer raw_outputs()")
        if "final_positions" not in env.raw_outputs():
            raise ValueError("a GeodesicShaper needs where episodes ended: build the env with final_positions=True")
        if len(self.env_agents) > _learn_native.RENDER_MAX_AGENTS:
            raise ValueError(f"at most {_learn_native.RENDER_MAX_AGENTS} agents per env")
        cop = lambda a: a.startswith("cop")
        scale = lambda a: float(scale_cop if cop(a) else scale_thief)
        self.agents = [a for a in self.env_agents if a in chosen and scale(a) != 0.0]
        if len(self.agents) > _learn_native.NAV_MAX_NAVIGATORS:
            raise ValueError(f"at most {_learn_native.NAV_MAX_NAVIGATORS} shaped agents per shaper (cat_render_nav_shape), not {len(self.agents)}")
        self.rows = [chosen.index(a) for a in self.agents]          # the row of ``agents`` (as given) each shaped agent stands in
        self.indices = [self.env_agents.index(a) for a in self.agents]
        self.opponent_masks = [sum(1 << j for j, b in enumerate(self.env_agents) if cop(b) != cop(a)) for a in self.agents]
        self.coef = [-scale(a) if cop(a) else scale(a) for a in self.agents]
        self.gamma, self.cap = float(gamma), cap
        self.N, self.G, self.given = env.num_envs, len(self.agents), len(chosen)
        self.field = field if field is not None else NavField.from_env(env, arena=True)
        if self.field.device != self.device or tuple(self.field.slot_map.shape) != (self.N,):
            raise ValueError(f"the field must lie on {self.device} with a slot_map of {self.N} slots")
        self.fused = self.device.type == "cuda"
        self.hops_prev = torch.full((self.G, self.N), -1, dtype=torch.int32, device=self.device)

    def _rows_of(self, t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
        """The [G, N] rows of the shaped agents: ``t`` itself, or their block of a tensor with one row per agent the constructor was given
        (cops come first in an env's order, so leaving a role out leaves one block)."""
        if t is None or tuple(t.shape) == (self.G, self.N):
            return t
        r0 = self.rows[0]
        if tuple(t.shape) == (self.given, self.N) and self.rows == list(range(r0, r0 + self.G)):
            return t[r0:r0 + self.G]
        raise ValueError(f"{name} must be fp32 [{self.G}, {self.N}], one row per shaped agent {self.agents}, or [{self.given}, {self.N}] "
                         f"with those agents in consecutive rows; got {tuple(t.shape)}")

    @torch.no_grad()
    def prime(self, raw) -> None:
        """``hops_prev`` = the separations of ``raw["team_positions"]``: the state the next ``step`` starts from."""
        if self.G == 0:
            return
        tp = raw["team_positions"]
        if self.fused:
            _learn_native.nav_shape(tp, self.field, self.indices, self.opponent_masks, self.coef, self.gamma, self.cap, self.hops_prev, prime=True)
        else:
            shaping_step(tp.to(self.device), None, None, None, self.field, self.indices, self.opponent_masks, self.coef, self.gamma, self.cap,
                         self.hops_prev, prime=True)

    @torch.no_grad()
    def step(self, raw, reward_rows: torch.Tensor, shaping_rows: Optional[torch.Tensor] = None) -> None:
        """One tick after the env's: ``reward_rows`` fp32 [G, N] (contiguous rows, any row stride) takes ``+ F``, ``shaping_rows`` (where
        given) ``F``; reads ``team_positions``, ``final_positions``, ``terminated`` and ``truncated`` of ``raw`` (the env's output buffers
        after the step)."""
        if self.G == 0:
            return
        rew, shp = self._rows_of(reward_rows, "reward_rows"), self._rows_of(shaping_rows, "shaping_rows")
        if self.fused:
            _learn_native.nav_shape(raw["team_positions"], self.field, self.indices, self.opponent_masks, self.coef, self.gamma, self.cap,
                                    self.hops_prev, final_positions=raw["final_positions"], terminated=raw["terminated"],
                                    truncated=raw["truncated"], reward_out=rew, shaping_out=shp)
        else:
            to = lambda t: t.to(self.device)
            shaping_step(to(raw["team_positions"]), to(raw["final_positions"]), to(raw["terminated"]), to(raw["truncated"]), self.field,
                         self.indices, self.opponent_masks, self.coef, self.gamma, self.cap, self.hops_prev, rew, shp)
