"""A geodesic start-state curriculum (a reverse curriculum: episodes start near the goal and move outwards as the learner succeeds):
slots whose episode just ended respawn with every cop a chosen number of shortest-path hops from a thief, on the hop table of
``navigation.NavField``.  PRIVILEGED information (the map and every agent's true position) reaches a policy only through WHERE its
episodes start: no observation, no reward, no flag changes.

    spawner = GeodesicSpawner(env, 2, 6)                     # every slot: each cop 2 .. 6 hops from its nearest thief
    env.set_spawner(spawner)                                 # VecCopsEnv respawns terminal slots inside step / step_raw
    ...
    spawner.adapt(0.3, 0.7, hi_max=64)                       # host rule: move ``hi`` with the cops' win rate since the last call

``navigation.spawn_step`` IS the rule (torch, any device); on a GPU ``respawn`` is one launch of ``cat_render_nav_spawn``
(include/cat_render.h), which equals it exactly, followed by one masked ``cat_reset`` launch of the env core with the chosen positions
(its workgroups without a masked slot leave before staging the map).  Both are capturable: no allocation of their own, no
synchronisation.  A slot the rule cannot serve (an empty band around the drawn thief) keeps the map's own spawn.

A respawned slot's ``reset_count`` advances twice per episode (the tick's auto-reset, then the masked reset): that shifts the Philox
spawn stream of the slot and nothing else.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .. import _learn_native
from ..navigation import BAND_MAX, NavField, spawn_step


def check_band(lo, hi) -> Tuple[int, int]:
    """(lo, hi) as ints; ValueError for anything but integers with ``1 <= lo <= hi <= 65534``."""
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"a band is two integer hop counts, got {(lo, hi)!r}")
    if not 1 <= lo <= hi <= BAND_MAX:
        raise ValueError(f"a band needs 1 <= lo <= hi <= {BAND_MAX}, got {(lo, hi)!r}")
    return int(lo), int(hi)


class GeodesicSpawner:
    """The curriculum state over ``env``: ``band`` int32 [N, 2] on the device -- (lo, hi) per slot, (-1, -1) = off: the slot keeps the
    map's own spawn -- and the int64 device counters ``ended`` (terminated rows seen by ``respawn``), ``cop_wins`` (of those, ``winner ==
    0``), ``requested`` (rows handed to the rule: terminated and not off) and ``placed_total`` (rows it placed).

    ``slots``: a slice or an index tensor of the slots that take the band (default: all); every other slot is off.  ``field``: a
    ``NavField`` of the env to share (else ``NavField.from_env(env, arena=True)``; it must be the arena field, see ``navigation``).
    ``lo`` / ``hi`` of the last ``set_band`` / ``adapt`` are kept as attributes (what a checkpoint stores)."""

    def __init__(self, env, lo: int, hi: int, *, field: Optional[NavField] = None, slots=None):
        self.device = torch.device(getattr(env, "device", "cpu"))
        agents = list(env.possible_agents)
        self.N, self.A = env.num_envs, len(agents)
        self.n_cops = sum(a.startswith("cop") for a in agents)
        if not 1 <= self.n_cops <= self.A - 1:
            raise ValueError(f"a GeodesicSpawner needs at least one cop and one thief, got {agents}")
        if self.A > _learn_native.RENDER_MAX_AGENTS:
            raise ValueError(f"at most {_learn_native.RENDER_MAX_AGENTS} agents per env")
        self._reset = getattr(env, "_spawn_reset", None)
        if self._reset is None:
            raise ValueError("a GeodesicSpawner resets the env core with chosen positions: the env must offer _spawn_reset(mask, positions)")
        self.field = field if field is not None else NavField.from_env(env, arena=True)
        if self.field.device != self.device or tuple(self.field.slot_map.shape) != (self.N,):
            raise ValueError(f"the field must lie on {self.device} with a slot_map of {self.N} slots")
        self.fused = self.device.type == "cuda"
        self.band = torch.full((self.N, 2), -1, dtype=torch.int32, device=self.device)
        self.positions = torch.zeros(self.N, self.A, 2, dtype=torch.float64, device=self.device)
        self.placed = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        self.ended, self.cop_wins, self.requested, self.placed_total = (torch.zeros((), dtype=torch.int64, device=self.device) for _ in range(4))
        self.lo, self.hi = check_band(lo, hi)
        self.last: Optional[Dict[str, int]] = None     # the counters as ``adapt`` last read them
        self.reset_placed: Optional[torch.Tensor] = None   # ``placed`` of the env's last explicit ``reset`` (a copy)
        self.set_band(lo, hi, slots)

    def _rows(self, slots):
        return slice(None) if slots is None else (slots if isinstance(slots, slice) else torch.as_tensor(slots, device=self.device))

    def set_band(self, lo: int, hi: int, slots=None) -> None:
        """``band[slots] = (lo, hi)`` in place (all slots by default): a captured graph follows it without a recapture."""
        self.lo, self.hi = check_band(lo, hi)
        self.band[self._rows(slots)] = torch.tensor([self.lo, self.hi], dtype=torch.int32, device=self.device)

    def set_off(self, slots=None) -> None:
        """``band[slots] = (-1, -1)``: those slots keep the map's own spawn."""
        self.band[self._rows(slots)] = -1

    @torch.no_grad()
    def place(self, mask: torch.Tensor, uniform: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rule on the slots of ``mask`` (u8 / bool [N]), then the masked reset of the env core with what it placed.  Returns
        ``placed`` (u8 [N], the spawner's own buffer)."""
        mask = mask.to(device=self.device, dtype=torch.uint8)
        if uniform is None:
            uniform = torch.rand(self.A, self.N, device=self.device)
        if self.fused:
            _learn_native.nav_spawn(mask.contiguous(), uniform.contiguous(), self.band, self.field, self.n_cops, self.positions, self.placed)
        else:
            spawn_step(mask, uniform.to(self.device), self.band, self.field, self.n_cops, self.positions, self.placed)
        self.requested += ((mask != 0) & (self.band[:, 0] >= 1)).sum()
        self.placed_total += self.placed.sum()
        self._reset(self.placed, self.positions)
        return self.placed

    def place_reset(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What an env's explicit ``reset`` calls after its own: ``place`` on the reset slots (None: all), and ``reset_placed`` keeps a copy
        of ``placed`` -- which first episodes started by the rule (``evaluate_by_separation`` reads it)."""
        placed = self.place(torch.ones(self.N, dtype=torch.uint8, device=self.device) if mask is None else mask)
        self.reset_placed = placed.clone()
        return placed

    @torch.no_grad()
    def respawn(self, raw, uniform: Optional[torch.Tensor] = None) -> torch.Tensor:
        """After a tick: the slots with ``raw["terminated"]`` are placed by the rule (``uniform`` fp32 [A, N], default ``torch.rand``) and
        the counters take the tick in.  ``reward``, ``terminated``, ``truncated``, ``winner`` and a bound ``final_positions`` buffer stay
        the terminal tick's: the masked reset stores none of them."""
        term = torch.as_tensor(raw["terminated"]).to(self.device) != 0
        self.ended += term.sum()
        self.cop_wins += (term & (torch.as_tensor(raw["winner"]).to(self.device) == 0)).sum()
        return self.place(term, uniform)

    def counters(self, clear: bool = False) -> Dict[str, int]:
        """The four counters as ints (one synchronisation)."""
        names = ("ended", "cop_wins", "requested", "placed_total")
        values = torch.stack([getattr(self, k) for k in names]).cpu().tolist()
        if clear:
            for k in names:
                getattr(self, k).zero_()
        return dict(zip(names, (int(v) for v in values)))

    def adapt(self, low: float, high: float, step: int = 1, hi_min: Optional[int] = None, hi_max: Optional[int] = None) -> int:
        """The host rule, on the counters since the last call (which it clears): with ``w = cop_wins / ended`` -- no change when
        ``ended == 0`` -- ``w > high`` raises the ``hi`` of every active slot by ``step`` (up to ``hi_max``), ``w < low`` lowers it (down
        to ``max(lo, hi_min)`` of the slot).  Integers only: ``w > high`` is decided as ``cop_wins > high * ended`` on the counts.  Returns the new ``hi``
        (the largest over the active slots)."""
        if isinstance(step, bool) or not isinstance(step, int) or step < 1:
            raise ValueError(f"step must be an integer >= 1, got {step!r}")
        if not 0.0 <= low <= high <= 1.0:
            raise ValueError(f"adapt needs 0 <= low <= high <= 1, got {(low, high)!r}")
        top = BAND_MAX if hi_max is None else min(int(hi_max), BAND_MAX)
        c = self.last = self.counters(clear=True)
        move = 0
        if c["ended"] > 0:
            move = step if c["cop_wins"] > high * c["ended"] else (-step if c["cop_wins"] < low * c["ended"] else 0)
        if move:
            lo, hi = self.band[:, 0], self.band[:, 1]
            active = lo >= 1
            floor = lo if hi_min is None else lo.clamp(min=int(hi_min))
            if move > 0:                # (a slot already beyond the bound stays where it is)
                new = torch.minimum(hi + move, hi.clamp(min=top))
            else:
                new = torch.maximum(hi + move, torch.minimum(hi, floor))
            self.band[:, 1] = torch.where(active, new, hi)
        active = self.band[:, 0] >= 1
        if bool(active.any()):
            self.hi = int(self.band[:, 1][active].max())
        return self.hi
