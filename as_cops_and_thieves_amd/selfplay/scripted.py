"""Scripted opponents: a deterministic, parameter-free yardstick for each role that is stronger than a coin flip -- a cop that heads for a
thief it sees and keeps heading for where it last saw one (``"chase"``), a thief that runs from a cop it sees towards open space
(``"evade"``).  Both read only what the learned policies read (an agent's own ray fan: ``distance`` f16 and ``object_type`` u8), avoid walls
by it and wander when they see nothing.

    actor = ScriptedActor(env, {"thief_0": "evade"})            # the thieves of a 2v1 env
    trainer.set_opponent("thief", actor)                        # the cops train against it; the rollout stays one captured graph
    actions = actor.act(env, starts)                            # or on its own: writes its agents' columns of [N, A]

``scripted_step`` below IS the rule (torch, any device); on a GPU ``ScriptedActor`` runs it as one launch of ``cat_rollout_scripted``
(include/cat_rollout.h), which equals it bit for bit.

The rule, per row = (scripted agent g, env n), from the R ray distances d[r] (non-negative, finite) and types t[r], one uniform u in
[0, 1) and the row's state (valid, heading, mem_ray, ttl):

* geometry in integers: ray r points at angle 2 pi r / R; actions 0 = -x, 1 = +y, 2 = +x, 3 = -y.  q(r) = ((8r + R) mod 8R) div 2R is
  the quadrant of r (quadrant k centred on k pi / 2, half-open), lean(r) = +1 if (8r + R) mod 2R >= R else -1 says towards which
  neighbouring quadrant r lies, o(r) = ((16r + R) mod 16R) div 2R is its octant, and the CONE of quadrant k is {r : o(r) == 2k}.
  ``ACT`` = (2, 1, 0, 3) maps a quadrant to its action and an action to its quadrant.  free[k] = min of d over the cone's rays that do NOT
  show the target type, +inf if there is none.
* sight: among the rays with t[r] == target the smallest key (bits16(d[r]) << 16) | r wins (nearest, lowest index on ties): mem_ray = r,
  ttl = memory_ticks, bearing b = r.  Otherwise, if ttl > 0: ttl -= 1, b = mem_ray.  Otherwise no bearing.
* with a bearing: k0 = q(b) (chase) or q(b) + 2 (evade), s = lean(b), order = [k0, k0 + s, k0 - s, k0 + 2] mod 4.
* without: h = min(3, int(4u)) on a row's first tick (valid == 0; no turn then), else the heading; turn = valid and u < turn_prob;
  side = +1 if bit 0 of uint32(u * 2^24) is set else -1; kh = ACT[h]; order = [kh, kh + side, kh - side, kh + 2] or, on a turn,
  [kh + side, kh - side, kh, kh + 2].
* choice: the first k of the order with free[k] >= clear_min, else the k with the largest free[k] (the earliest on ties).
  action = ACT[k]; the state becomes (1, action, mem_ray, ttl).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _learn_native

SCRIPTS = {"chase": 0, "evade": 1}
COP, THIEF = 1, 2                   # constants.ObjectType: what a thief / a cop looks for
ACT = (2, 1, 0, 3)
_NO_KEY = 1 << 40


@dataclasses.dataclass(frozen=True)
class ScriptedParams:
    memory_ticks: int = 30          # ticks a lost bearing is still followed
    clear_min: float = 12.0         # a cone is free when nothing but the target is closer than this
    turn_prob: float = 0.02         # chance per tick of a turn while wandering

    def __post_init__(self):
        if not (isinstance(self.memory_ticks, int) and self.memory_ticks >= 0):
            raise ValueError(f"memory_ticks must be an int >= 0: {self.memory_ticks!r}")
        if not float(self.clear_min) >= 0.0:
            raise ValueError(f"clear_min must be a number >= 0: {self.clear_min!r}")
        if not 0.0 <= float(self.turn_prob) <= 1.0:
            raise ValueError(f"turn_prob must lie in [0, 1]: {self.turn_prob!r}")


def target_of(agent: str) -> int:
    """The type code ``agent`` (``cop_i`` / ``thief_j``) looks for: the other team's."""
    return THIEF if agent.startswith("cop") else COP


def script_code(name) -> int:
    """"chase" / "evade" -> the kernel's code; None -> -1 (not scripted there).  ValueError otherwise."""
    if name is None:
        return -1
    if isinstance(name, str) and name in SCRIPTS:
        return SCRIPTS[name]
    raise ValueError(f"{name!r} is not a script: {sorted(SCRIPTS)} or None")


@torch.no_grad()
def scripted_step(distance: torch.Tensor, obj_type: torch.Tensor, uniform: torch.Tensor, state: torch.Tensor, keep: Optional[torch.Tensor],
                  script: torch.Tensor, target: torch.Tensor, params: ScriptedParams = ScriptedParams()) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rule of the module docstring on rows of any leading shape ``[...]``: distance f16 ``[..., R]``, obj_type u8 ``[..., R]``, uniform
    fp32, state int32 ``[..., 4]``, keep (bool or number, 0 = take the state as zero) or None, script and target integer tensors, each
    broadcastable to ``[...]``.  Returns (action int32 ``[...]``, new state int32 ``[..., 4]``); where script is -1 the action is -1 and the
    state is the one passed in.  Nothing is modified in place."""
    R = distance.shape[-1]
    if not 8 <= R <= 1024:
        raise ValueError(f"{R} rays: 8..1024 are allowed")
    assert distance.dtype == torch.float16 and obj_type.dtype == torch.uint8 and obj_type.shape == distance.shape
    assert uniform.dtype == torch.float32 and state.dtype == torch.int32 and state.shape == distance.shape[:-1] + (4,)
    dev, shape = distance.device, distance.shape[:-1]
    i64 = torch.int64
    script = torch.as_tensor(script, device=dev).to(i64).expand(shape)
    target = torch.as_tensor(target, device=dev).to(i64).expand(shape)
    uniform = uniform.expand(shape)
    act_t = torch.tensor(ACT, dtype=i64, device=dev)
    r = torch.arange(R, dtype=i64, device=dev)
    octant = ((16 * r + R) % (16 * R)) // (2 * R)
    is_target = obj_type.to(i64) == target.unsqueeze(-1)

    # free[k]: f16 -> fp32 is exact
    d32 = distance.float()
    inf = torch.full_like(d32, float("inf"))
    free = torch.stack([torch.where((octant == 2 * k) & ~is_target, d32, inf).min(dim=-1).values for k in range(4)], dim=-1)       # [..., 4]

    # sight
    bits = distance.view(torch.int16).to(i64) & 0xFFFF
    key = torch.where(is_target, (bits << 16) | r, torch.full_like(bits, _NO_KEY)).min(dim=-1).values
    seen = key < _NO_KEY
    st = state.to(i64)
    if keep is not None:
        st = st * (torch.as_tensor(keep, device=dev) != 0).to(i64).expand(shape).unsqueeze(-1)
    valid, heading, mem, ttl = st.unbind(-1)
    remembered = ~seen & (ttl > 0)
    mem = torch.where(seen, key & 0xFFFF, mem)
    ttl = torch.where(seen, torch.full_like(ttl, params.memory_ticks), torch.where(remembered, ttl - 1, ttl))
    bearing = seen | remembered
    b = mem                                                                    # the bearing where there is one

    # the order with a bearing
    q = ((8 * b + R) % (8 * R)) // (2 * R)
    lean = torch.where(((8 * b + R) % (2 * R)) >= R, 1, -1)
    k0 = torch.where(script == SCRIPTS["evade"], q + 2, q)
    with_b = torch.stack([k0, k0 + lean, k0 - lean, k0 + 2], dim=-1)
    # and without
    first = valid == 0
    h = torch.where(first, (4.0 * uniform).to(i64).clamp(max=3), heading & 3)
    turn = ~first & (uniform < torch.tensor(params.turn_prob, dtype=torch.float32, device=dev))
    side = torch.where(((uniform * 16777216.0).to(i64) & 1) == 1, 1, -1)
    kh = act_t[h]
    straight = torch.stack([kh, kh + side, kh - side, kh + 2], dim=-1)
    turned = torch.stack([kh + side, kh - side, kh, kh + 2], dim=-1)
    without_b = torch.where(turn.unsqueeze(-1), turned, straight)
    order = torch.where(bearing.unsqueeze(-1), with_b, without_b) % 4          # [..., 4]

    # choice
    f = free.gather(-1, order)
    j = torch.arange(4, dtype=i64, device=dev).expand_as(order)
    ok = f >= torch.tensor(params.clear_min, dtype=torch.float32, device=dev)
    first_ok = torch.where(ok, j, torch.full_like(j, 4)).min(dim=-1).values
    largest = torch.where(f == f.max(dim=-1, keepdim=True).values, j, torch.full_like(j, 4)).min(dim=-1).values
    pick = torch.where(first_ok < 4, first_ok, largest)
    action = act_t[order.gather(-1, pick.unsqueeze(-1)).squeeze(-1)]

    on = script >= 0
    new = torch.stack([torch.ones_like(action), action, mem, ttl], dim=-1).to(torch.int32)
    return torch.where(on, action, torch.full_like(action, -1)).to(torch.int32), torch.where(on.unsqueeze(-1), new, state)


class ScriptedActor:
    """Scripted agents over ``env`` with the opponent surface ``MAPPOTrainer.set_opponent`` duck-types (``agents``, ``env_agents``, ``N``,
    ``R``, ``device``, ``fused``, ``table``, ``actions``, ``segments``, ``reset``, ``get_state`` / ``set_state``, ``act``).

    ``scripts``: {agent: "chase" | "evade"} for every agent the actor plays everywhere (the plain form, one segment); ``agents``: the agents
    it covers, in the env's order (default: the keys of ``scripts``) -- ``set_segments`` then says per row range which of them follows which
    script, None leaving an agent's column and state alone there.

    ``fused`` is True on a GPU: per tick one ``torch.rand(G, N)`` and ONE launch of ``cat_rollout_scripted``, capturable; elsewhere the
    torch form ``scripted_step`` on the observation dictionaries, from the same single ``torch.rand(G, N)``."""

    def __init__(self, env, scripts: Optional[Dict[str, Optional[str]]] = None, agents: Optional[Sequence[str]] = None,
                 params: ScriptedParams = ScriptedParams(), device=None):
        self.device = torch.device(device) if device is not None else torch.device(getattr(env, "device", "cpu"))
        self.env_agents = list(env.possible_agents)
        scripts = dict(scripts or {})
        chosen = list(scripts) if agents is None else list(agents)
        if not chosen or len(set(chosen)) != len(chosen) or any(a not in self.env_agents for a in chosen):
            raise ValueError(f"agents must be a non-empty subset of the env's agents {self.env_agents} without repeats: {chosen}")
        if any(a not in chosen for a in scripts):
            raise ValueError(f"scripts name agents the actor does not cover: {sorted(set(scripts) - set(chosen))}")
        self.agents: List[str] = [a for a in self.env_agents if a in chosen]
        if len(self.agents) > 8:
            raise ValueError("at most 8 scripted agents")
        self.indices = [self.env_agents.index(a) for a in self.agents]
        self.targets = [target_of(a) for a in self.agents]
        self.N = env.num_envs
        self.R = env.observation_spaces[self.agents[0]]["distance"].shape[0]
        if not _learn_native.SCRIPTED_MIN_RAYS <= self.R <= _learn_native.SCRIPTED_MAX_RAYS:
            raise ValueError(f"{self.R} rays: {_learn_native.SCRIPTED_MIN_RAYS}..{_learn_native.SCRIPTED_MAX_RAYS} are allowed")
        self.params = params
        self.G = len(self.agents)
        self.fused = self.device.type == "cuda"
        if self.fused and not hasattr(env, "raw_outputs"):
            raise ValueError("a ScriptedActor on a GPU reads the env core's observation buffers: the env must offer raw_outputs()")
        self.actions = torch.zeros(self.N, len(self.env_agents), dtype=torch.int32, device=self.device)
        self.state = torch.zeros(self.G, self.N, 4, dtype=torch.int32, device=self.device)
        self._keep = torch.zeros(self.N, dtype=torch.float32, device=self.device)
        self._index_t = torch.tensor(self.indices, dtype=torch.long, device=self.device)
        self._target_t = torch.tensor(self.targets, dtype=torch.int64, device=self.device).view(self.G, 1)
        self.table = None
        self.set_segments([(0, self.N, {a: scripts.get(a) for a in self.agents})])

    def set_segments(self, segments) -> None:
        """``segments``: [(start, stop, {agent: "chase" | "evade" | None}), ...] -- contiguous row ranges that cover 0 .. N in order, every
        agent of the actor named in each.  The rules of ``cat_rollout_scripted``; ValueError otherwise (the current table then stays).  A
        new table is a new ``table`` object: a trainer that captured a rollout with the old one recaptures."""
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
                rows[g].append(script_code(who[a]))
        self._set_table(_learn_native.scripted_table(self.N, self.G, bounds, rows))

    def _set_table(self, table) -> None:
        self.table = table
        script = torch.empty(self.G, self.N, dtype=torch.int64)
        for s, (lo, hi) in enumerate(zip(table.start[:-1], table.start[1:])):
            for g in range(self.G):
                script[g, lo:hi] = table.rows[g][s]
        self._script_t = script.to(self.device)

    @property
    def segments(self) -> List[Tuple[int, int]]:
        """[(start, stop)] of the current table."""
        b = self.table.start
        return list(zip(b[:-1], b[1:]))

    # ------------------------------------------------------------------ state
    @torch.no_grad()
    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Forget every slot's heading and bearing, or those of the slots where ``mask`` (bool [N]) is set."""
        if mask is None:
            self.state.zero_()
        else:
            self.state.masked_fill_(mask.view(1, -1, 1), 0)

    def get_state(self, out=None):
        if out is None:
            return self.state.clone()
        out.copy_(self.state)
        return out

    def set_state(self, state) -> None:
        self.state.copy_(state)

    # ------------------------------------------------------------------ the act tick
    def _check_actions(self, actions):
        if actions is None:
            return self.actions
        if not (actions.dtype == torch.int32 and tuple(actions.shape) == tuple(self.actions.shape) and actions.is_contiguous()
                and actions.device == self.actions.device):
            raise ValueError(f"actions must be a contiguous int32 {tuple(self.actions.shape)} tensor on {self.actions.device}")
        return actions

    @torch.no_grad()
    def act(self, env, starts: Optional[torch.Tensor] = None, obs=None, actions: Optional[torch.Tensor] = None, uniform=None) -> torch.Tensor:
        """The scripted agents' actions for the env's current observations, into their columns of ``actions`` (int32 [N, A] over ALL the
        env's agents; default ``self.actions``), which is returned; no other column is touched.  ``starts`` (bool [N]): an episode starts in
        these slots, their state is taken as zero; None carries every state.  ``obs``: the env's observation dictionaries (torch form
        only; fetched when omitted).  ``uniform`` fp32 [G, N]: the tick's numbers instead of a fresh ``torch.rand(G, N)``."""
        actions = self._check_actions(actions)
        u = torch.rand(self.G, self.N, device=self.device) if uniform is None else uniform
        if self.fused:
            keep = None if starts is None else torch.logical_not(starts, out=self._keep)
            _learn_native.rollout_scripted(env.raw_outputs(), self.indices, self.targets, self.table, u, keep, self.state, actions,
                                           self.params.memory_ticks, self.params.clear_min, self.params.turn_prob)
            return actions
        if obs is None:
            obs = env.observations() if hasattr(env, "observations") else env._obs()
        d = torch.stack([obs[a]["distance"] for a in self.agents]).to(self.device)
        t = torch.stack([obs[a]["object_type"] for a in self.agents]).to(self.device)
        keep = None if starts is None else (~starts).view(1, self.N)
        act, new = scripted_step(d, t, u, self.state, keep, self._script_t, self._target_t, self.params)
        self.state.copy_(new)
        cols = actions.index_select(1, self._index_t)
        actions.index_copy_(1, self._index_t, torch.where(act.t() >= 0, act.t(), cols))
        return actions
