"""Position statistics: where the agents spend their time, added up where the data lies.

The env core writes, every tick, ``team_positions`` (f16 ``[N, A, 2]``), ``obs_type`` (u8 ``[N, A, R]``) and ``terminated`` per slot
(``rollout_fused`` writes the same with a leading T).  ``PositionTracker`` owns the count maps of ``include/cat_render.h``
(``cat_render_positions_update``) on a grid of ``cell x cell`` pixels and adds those rows into them: on a GPU device one kernel launch
per ``update`` on the current stream (no host synchronisation: it can be captured in a HIP graph with the env tick it follows), on CPU
tensors the NumPy form below, which DEFINES every number -- all sums are integers, so the two agree exactly.

The counting rule, for row t of slot n with ``g = group[n]``:

1. the row is skipped if ``g`` is no group (``-1``), or if ``done[n] >= quota[n]``;
2. otherwise ``rows[g] += 1`` and, for every agent a with ``(x, y)`` the f16 values of ``team_positions[t, n, a]``: the position is
   valid iff both are finite, ``x >= 0``, ``y >= 0``, ``cx = int(floor(x)) // cell < Wc`` and ``cy = int(floor(y)) // cell < Hc``;
   an invalid one adds to ``outside[g, a]``; a valid one on a terminal row adds to ``counts[g, SPAWN, a, cx, cy]``; a valid one on any
   other row adds to ``counts[g, OCC, a, cx, cy]`` and, if ``obs_type`` is given and ``seen(a)`` holds, to ``counts[g, SEEN, a, cx, cy]``;
3. finally ``done[n] += terminated[t, n] != 0``.

With auto-reset the env resets a slot INSIDE its terminal tick, so a terminal row's buffers hold the first observation of the new episode:
that is why such a row counts as a spawn.  A frame-skip row (``step_raw(actions, repeat=k)``) counts once: one count per decision, at the
window's last position.

Where an episode ENDED is a separate input: the env core's end-of-episode positions (``CatSim.bind_final_positions``: on a terminal row the
tick-start positions of the episode that ended -- the ones the termination check read -- any other row holds nothing to read).  A tracker
built with ``final_positions=True`` and fed ``update(..., final_positions=, truncated=)`` also keeps ``ends`` int64 ``[G, 2, A, Wc, Hc]``
(planes ``CAPTURE`` / ``TIMEOUT``) and ``ends_outside`` ``[G, 2, A]`` (``cat_render_positions_ends_update``).  The ends rule, for row t of
slot n (``_update_ends_host`` defines it):

1. the row is skipped exactly when rule 1 above skips it (``done[n]`` as it stands BEFORE this row);
2. otherwise, if ``terminated[t, n] != 0``: plane = ``TIMEOUT`` if ``truncated[t, n] != 0`` else ``CAPTURE``, and for every agent a the
   f16 pair ``final_positions[t, n, a]`` is valid by the rule above; an invalid one adds to ``ends_outside[g, plane, a]``, a valid one to
   ``ends[g, plane, a, cx, cy]``.  A row that is not terminal adds nothing and its ``final_positions`` are never read.

So a slot's ``quota``-th terminal row is the last whose end is counted, as it is the last whose spawn is.

``seen(a)`` is ROLE-LEVEL: it holds when some agent of the other role has a ray whose ``obs_type`` is a's role code (``COP`` for a cop,
``THIEF`` for a thief).  With two agents of one role it says "an agent of my role is in an opponent's sight"; ``obs_type`` cannot tell
which one (``hit_shape`` could, but it is a debug output that is off by default).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _learn_native as ln
from .constants import ObjectType

OCC, SEEN, SPAWN = ln.POSITIONS_OCC, ln.POSITIONS_SEEN, ln.POSITIONS_SPAWN
PLANES = ("occ", "seen", "spawn")
CAPTURE, TIMEOUT = ln.POSITIONS_CAPTURE, ln.POSITIONS_TIMEOUT
END_PLANES = ("capture", "timeout")
INT32_MAX = 2 ** 31 - 1
_COP, _THIEF = ObjectType.COP.value, ObjectType.THIEF.value


def grid_shape(window, cell: int):
    """``(Wc, Hc)`` of a ``W x H`` pixel window cut into ``cell x cell`` cells (the last column / row may be narrower)."""
    W, H = int(window[0]), int(window[1])
    return -(-W // cell), -(-H // cell)


class PositionTracker:
    """Per-group occupancy / exposure / spawn maps (``include/cat_render.h`` ``cat_render_positions_update``).

    ``agents``: the env's agent ids, cops first (``n_cops`` of them); ``window``: ``(W, H)`` pixels, the largest ``int(window)`` over
    the batch's maps; ``cell``: cell size in pixels; ``n_groups``: G.  Every slot starts in group 0 without a quota.
    ``final_positions=True``: the tracker also keeps the capture / timeout maps (``ends``, ``ends_outside``) and ``update`` takes the
    end-of-episode positions; without it nothing of that exists and every result is the same as before, key for key."""

    def __init__(self, num_envs: int, agents: Sequence[str], n_cops: int, window, cell: int, n_groups: int = 1, device=None,
                 final_positions: bool = False):
        self.N, self.agents, self.A, self.n_cops = int(num_envs), list(agents), len(agents), int(n_cops)
        self.G = int(n_groups)
        if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or cell < 1:
            raise ValueError(f"PositionTracker: cell must be an integer number of pixels >= 1, got {cell!r}")
        self.cell = int(cell)
        self.W, self.H = int(window[0]), int(window[1])
        if self.N < 1 or not 1 <= self.A <= ln.RENDER_MAX_AGENTS or not 0 <= self.n_cops <= self.A or self.G < 1 or self.W < 1 or self.H < 1:
            raise ValueError(f"PositionTracker: num_envs >= 1, 1..{ln.RENDER_MAX_AGENTS} agents, 0 <= n_cops <= agents, n_groups >= 1 and a "
                             "window of at least 1 x 1 are required")
        self.Wc, self.Hc = grid_shape((self.W, self.H), self.cell)
        self.device = torch.device("cpu" if device is None else device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        G, A, N = self.G, self.A, self.N
        # ONE allocation: counts, outside, rows and (as int32) done -- counts() brings all of them to the host in one copy
        # (with final_positions: ends and ends_outside behind them)
        n_counts, n_out = G * 3 * A * self.Wc * self.Hc, G * A
        self.final_positions = bool(final_positions)
        n_base = n_counts + n_out + G + (N + 1) // 2
        n_ends, n_eout = (G * 2 * A * self.Wc * self.Hc, G * 2 * A) if self.final_positions else (0, 0)
        self._flat = torch.zeros(n_base + n_ends + n_eout, dtype=torch.int64, device=self.device)
        self._counts = self._flat[:n_counts].view(G, 3, A, self.Wc, self.Hc)
        self._outside = self._flat[n_counts:n_counts + n_out].view(G, A)
        self._rows = self._flat[n_counts + n_out:n_counts + n_out + G]
        self._done = self._flat[n_counts + n_out + G:n_base].view(torch.int32)[:N]
        self._ends = self._flat[n_base:n_base + n_ends].view(G, 2, A, self.Wc, self.Hc) if self.final_positions else None
        self._ends_outside = self._flat[n_base + n_ends:].view(G, 2, A) if self.final_positions else None
        # ONE group and ONE quota buffer for the tracker's life: the update launch takes their pointers by value, so a launch captured
        # in a HIP graph keeps reading them, and set_groups / set_quota after the capture reach the replays
        self._group = torch.zeros(N, dtype=torch.int32, device=self.device)
        self._quota = torch.full((N,), INT32_MAX, dtype=torch.int32, device=self.device)
        self._gpu = self.device.type == "cuda"
        self._last = (None, None)     # (what the last one-launch update was given, its checked argument blocks: ends or None, positions)
        if self._gpu:
            ln.lib()     # a missing kernel library is an error here, not at the first update

    # ------------------------------------------------------------------ groups and quota
    def set_groups(self, groups=None, *, bounds=None) -> None:
        """The group of every slot: ``groups`` an int array ``[N]`` with values in ``-1 .. n_groups - 1`` (-1 = not counted), or
        ``bounds`` = S + 1 row bounds of S <= n_groups contiguous segments (``_learn_native.segment_bounds``), segment s being group s.
        Neither: every slot in group 0.  Copied into the tracker's own buffer, so it also reaches captured update launches."""
        if groups is not None and bounds is not None:
            raise ValueError("set_groups: give the per-slot groups or the segment bounds, not both")
        if bounds is not None:
            start = ln.segment_bounds(self.N, bounds)
            if len(start) - 1 > self.G:
                raise ValueError(f"set_groups: {len(start) - 1} segments but the tracker has {self.G} groups")
            g = np.repeat(np.arange(len(start) - 1, dtype=np.int32), np.diff(start))
        elif groups is None:
            g = np.zeros(self.N, dtype=np.int32)
        else:
            g = torch.as_tensor(groups).detach().cpu().numpy().reshape(-1)
            if g.shape != (self.N,) or g.dtype.kind not in "iu":
                raise ValueError(f"set_groups: expected {self.N} integers, got {g.shape} {g.dtype}")
            if g.size and (g.min() < -1 or g.max() >= self.G):
                raise ValueError(f"set_groups: groups must lie in -1 .. {self.G - 1}")
            g = g.astype(np.int32)
        self._group.copy_(torch.from_numpy(np.ascontiguousarray(g)))

    def set_quota(self, quota) -> None:
        """How many terminal rows of each slot are followed (the slot's rows after its ``quota``-th terminal row are skipped): an int
        (every slot), an int tensor / sequence ``[N]``, or None (no limit).  Copied into the tracker's own buffer."""
        if quota is None or isinstance(quota, int):
            self._quota.fill_(INT32_MAX if quota is None else quota)
        else:
            self._quota.copy_(torch.as_tensor(quota).to(torch.int32).reshape(self.N))

    # ------------------------------------------------------------------ feeding
    def update(self, team_positions, terminated, obs_type=None, final_positions=None, truncated=None) -> None:
        """One row ``[N, ...]`` or T consecutive rows ``[T, N, ...]``: team_positions f16 ``[.., N, A, 2]``, terminated ``[.., N]`` (uint8
        or bool), obs_type u8 ``[.., N, A, R]`` or None (no SEEN plane).  ``final_positions`` f16 ``[.., N, A, 2]`` with ``truncated``
        ``[.., N]`` (both or neither; a tracker built with ``final_positions=True`` only): the same rows' end-of-episode positions, added to
        the capture / timeout maps (``update_ends``) before ``done`` advances over these rows.  An env feeds the same output buffers tick
        after tick: a call with the buffers of the one before (same addresses, shapes, strides and types) launches again from the checked
        argument blocks."""
        if (final_positions is None) != (truncated is None):
            raise ValueError("PositionTracker.update: final_positions and truncated go together")
        given = None
        if self._gpu:
            given = tuple(None if t is None else (t.data_ptr(), t.shape, t.stride(), t.dtype)
                          for t in (team_positions, terminated, obs_type, final_positions, truncated))
            if given == self._last[0]:
                if self._last[1][0] is not None:
                    ln.positions_ends_launch(self._last[1][0])
                ln.positions_launch(self._last[1][1])
                return
        eargs = None
        if final_positions is not None:      # first: it reads ``done`` as it stands before these rows
            eargs = self.update_ends(final_positions, terminated, truncated)
        if team_positions.dim() == 3:
            team_positions, terminated = team_positions[None], terminated[None]
            obs_type = None if obs_type is None else obs_type[None]
        T = team_positions.shape[0]
        if tuple(team_positions.shape) != (T, self.N, self.A, 2) or tuple(terminated.shape) != (T, self.N):
            raise ValueError(f"PositionTracker.update: expected [T, {self.N}, {self.A}, 2] positions and [T, {self.N}] flags, got "
                             f"{tuple(team_positions.shape)}, {tuple(terminated.shape)}")
        if obs_type is not None and (obs_type.dim() != 4 or tuple(obs_type.shape[:3]) != (T, self.N, self.A) or obs_type.shape[3] < 1):
            raise ValueError(f"PositionTracker.update: expected [T, {self.N}, {self.A}, R] obs_type, got {tuple(obs_type.shape)}")
        if any(t.device != self.device for t in (team_positions, terminated) + (() if obs_type is None else (obs_type,))):
            raise ValueError(f"PositionTracker.update: the rows must lie on {self.device}")
        team_positions = team_positions.to(torch.float16).contiguous()
        terminated = (terminated.view(torch.uint8) if terminated.dtype == torch.bool else terminated.to(torch.uint8)).contiguous()
        obs_type = None if obs_type is None else obs_type.to(torch.uint8).contiguous()
        if self._gpu:
            for t0 in range(0, T, ln.POSITIONS_MAX_TICKS):
                sl = slice(t0, min(T, t0 + ln.POSITIONS_MAX_TICKS))
                args = ln.positions_update(team_positions[sl], terminated[sl], None if obs_type is None else obs_type[sl], self._group, self._quota,
                                           self._counts, self._outside, self._rows, self._done, self.n_cops, self.cell)
            same = all(t is None or t.data_ptr() == g[0] for t, g in zip((team_positions, terminated, obs_type), given))   # nothing was converted
            same = same and (final_positions is None or eargs is not None)
            self._last = (given, (eargs, args)) if same and T <= ln.POSITIONS_MAX_TICKS else (None, None)
        else:
            self._update_host(team_positions.numpy(), terminated.numpy(), None if obs_type is None else obs_type.numpy())

    def update_ends(self, final_positions, terminated, truncated):
        """The capture / timeout maps alone (a tracker built with ``final_positions=True``): one row or T rows of end-of-episode positions
        f16 ``[.., N, A, 2]`` with their ``terminated`` / ``truncated`` flags ``[.., N]``, under the ends rule of the module docstring.
        ``done`` is read as it stands and not advanced -- ``update`` calls this first and then counts the same rows; a caller whose
        occupancy rows carry other flags (an env without auto-reset) calls it on its own.  On a GPU: one launch per 65536 rows; returns the
        launch's argument block if it can be repeated as it is (one launch, nothing converted), else None."""
        if not self.final_positions:
            raise ValueError("PositionTracker: this tracker was built without final_positions=True and keeps no capture / timeout maps")
        if final_positions.dim() == 3:
            final_positions, terminated, truncated = final_positions[None], terminated[None], truncated[None]
        T = final_positions.shape[0]
        if tuple(final_positions.shape) != (T, self.N, self.A, 2) or tuple(terminated.shape) != (T, self.N) or tuple(truncated.shape) != (T, self.N):
            raise ValueError(f"PositionTracker.update_ends: expected [T, {self.N}, {self.A}, 2] final positions and [T, {self.N}] flags, got "
                             f"{tuple(final_positions.shape)}, {tuple(terminated.shape)}, {tuple(truncated.shape)}")
        if any(t.device != self.device for t in (final_positions, terminated, truncated)):
            raise ValueError(f"PositionTracker.update_ends: the rows must lie on {self.device}")
        as_u8 = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).contiguous()
        before = tuple(t.data_ptr() for t in (final_positions, terminated, truncated))
        final_positions, terminated, truncated = final_positions.to(torch.float16).contiguous(), as_u8(terminated), as_u8(truncated)
        if not self._gpu:
            self._update_ends_host(final_positions.numpy(), terminated.numpy(), truncated.numpy())
            return None
        done = self._done
        for t0 in range(0, T, ln.POSITIONS_MAX_TICKS):
            sl = slice(t0, min(T, t0 + ln.POSITIONS_MAX_TICKS))
            if t0:      # a later chunk: the slots' terminal rows so far, carried along in a copy
                done = done + terminated[t0 - ln.POSITIONS_MAX_TICKS:t0].ne(0).sum(0, dtype=torch.int32)
            eargs = ln.positions_ends_update(final_positions[sl], terminated[sl], truncated[sl], self._group, self._quota, done,
                                             self._ends, self._ends_outside, self.cell)
        same = before == tuple(t.data_ptr() for t in (final_positions, terminated, truncated))
        return eargs if same and T <= ln.POSITIONS_MAX_TICKS else None

    def _update_ends_host(self, final_pos, terminated, truncated) -> None:
        """The ends rule in NumPy: slots in parallel, rows in order.  Reads ``done`` as it stands before these rows and leaves it alone
        (``_update_host`` over the same rows advances it): the count of a slot's terminal rows runs along in a copy."""
        ends, ends_outside = self._ends.numpy(), self._ends_outside.numpy()   # views
        group, quota, done = self._group.numpy(), self._quota.numpy(), self._done.numpy().copy()
        cell = self.cell
        agent = np.arange(self.A)[None, :]
        for t in range(final_pos.shape[0]):
            ends_here = (group >= 0) & (group < self.G) & (done < quota) & (terminated[t] != 0)
            idx = np.nonzero(ends_here)[0]
            done += ends_here
            if not idx.size:
                continue
            g = group[idx]
            plane = np.where(truncated[t, idx] != 0, TIMEOUT, CAPTURE)
            xy = final_pos[t, idx].astype(np.float32)
            x, y = xy[..., 0], xy[..., 1]
            valid = np.isfinite(x) & np.isfinite(y) & (x >= 0) & (y >= 0)
            cx = np.floor(np.where(valid, x, 0.0)).astype(np.int64) // cell
            cy = np.floor(np.where(valid, y, 0.0)).astype(np.int64) // cell
            valid &= (cx < self.Wc) & (cy < self.Hc)
            gg, pp, aa = (np.broadcast_to(v, valid.shape) for v in (g[:, None], plane[:, None], agent))
            np.add.at(ends_outside, (gg[~valid], pp[~valid], aa[~valid]), 1)
            np.add.at(ends, (gg[valid], pp[valid], aa[valid], cx[valid], cy[valid]), 1)

    def _update_host(self, pos, terminated, obs_type=None) -> None:
        """The counting rule in NumPy: slots in parallel, rows in order."""
        counts, outside, rows, done = self._counts.numpy(), self._outside.numpy(), self._rows.numpy(), self._done.numpy()   # views
        group, quota = self._group.numpy(), self._quota.numpy()
        nc, cell = self.n_cops, self.cell
        agent = np.arange(self.A)[None, :]
        for t in range(pos.shape[0]):
            idx = np.nonzero((group >= 0) & (group < self.G) & (done < quota))[0]
            if not idx.size:
                continue
            g = group[idx]
            np.add.at(rows, g, 1)
            term = terminated[t, idx] != 0
            xy = pos[t, idx].astype(np.float32)
            x, y = xy[..., 0], xy[..., 1]
            valid = np.isfinite(x) & np.isfinite(y) & (x >= 0) & (y >= 0)
            cx = np.floor(np.where(valid, x, 0.0)).astype(np.int64) // cell
            cy = np.floor(np.where(valid, y, 0.0)).astype(np.int64) // cell
            valid &= (cx < self.Wc) & (cy < self.Hc)
            gg, aa = np.broadcast_to(g[:, None], valid.shape), np.broadcast_to(agent, valid.shape)
            np.add.at(outside, (gg[~valid], aa[~valid]), 1)
            spawn, occ = valid & term[:, None], valid & ~term[:, None]
            np.add.at(counts, (gg[spawn], SPAWN, aa[spawn], cx[spawn], cy[spawn]), 1)
            np.add.at(counts, (gg[occ], OCC, aa[occ], cx[occ], cy[occ]), 1)
            if obs_type is not None:
                types = obs_type[t, idx]
                sees_cop, sees_thief = (types == _COP).any(axis=-1), (types == _THIEF).any(axis=-1)
                seen = np.zeros(valid.shape, dtype=bool)
                seen[:, :nc] = sees_cop[:, nc:].any(axis=-1, keepdims=True)      # a cop is seen by the thieves
                seen[:, nc:] = sees_thief[:, :nc].any(axis=-1, keepdims=True)    # a thief by the cops
                seen &= occ
                np.add.at(counts, (gg[seen], SEEN, aa[seen], cx[seen], cy[seen]), 1)
            done[idx] += term

    def clear(self) -> None:
        """Zero the maps (the capture / timeout maps and ``ends_outside`` included), ``outside``, ``rows`` and the terminal rows counted
        towards the quota; the groups and the quota stay."""
        self._flat.zero_()

    # ------------------------------------------------------------------ reading
    def tensors(self) -> Dict[str, torch.Tensor]:
        """The buffers as they lie on the device (views of the tracker's state: no copy, no synchronisation)."""
        t = {"counts": self._counts, "outside": self._outside, "rows": self._rows, "done": self._done, "group": self._group,
             "quota": self._quota}
        if self.final_positions:
            t.update(ends=self._ends, ends_outside=self._ends_outside)
        return t

    def counts(self) -> Dict[str, np.ndarray]:
        """Host copies of ``counts`` int64 ``[G, 3, A, Wc, Hc]`` (planes OCC, SEEN, SPAWN; x-major like the frames), ``outside``
        ``[G, A]``, ``rows`` ``[G]`` and ``done`` int32 ``[N]``: one copy, one synchronisation.  A tracker built with
        ``final_positions=True`` adds ``ends`` int64 ``[G, 2, A, Wc, Hc]`` (planes CAPTURE, TIMEOUT) and ``ends_outside`` ``[G, 2, A]``."""
        flat = self._flat.cpu().numpy().copy()
        G, A, N = self.G, self.A, self.N
        n_counts, n_out = G * 3 * A * self.Wc * self.Hc, G * A
        n_base = n_counts + n_out + G + (N + 1) // 2
        c = {"counts": flat[:n_counts].reshape(G, 3, A, self.Wc, self.Hc), "outside": flat[n_counts:n_counts + n_out].reshape(G, A),
             "rows": flat[n_counts + n_out:n_counts + n_out + G], "done": flat[n_counts + n_out + G:n_base].view(np.int32)[:N]}
        if self.final_positions:
            n_ends = G * 2 * A * self.Wc * self.Hc
            c["ends"] = flat[n_base:n_base + n_ends].reshape(G, 2, A, self.Wc, self.Hc)
            c["ends_outside"] = flat[n_base + n_ends:].reshape(G, 2, A)
        return c

    def summary(self) -> List[Dict[str, object]]:
        """Per group: ``rows`` and, per agent id, ``outside``, ``occupied`` / ``seen`` / ``spawns`` (the planes' sums), ``cells_visited``
        (cells with OCC > 0), ``seen_fraction`` = sum(SEEN) / sum(OCC) (0 without occupancy) and the argmax cells ``(cx, cy)`` of OCC
        (``top_cell``) and of OCC - SEEN (``top_hidden_cell``, the most-used hidden cell); None where the plane is all zero.  A tracker
        built with ``final_positions=True`` adds ``captures`` / ``timeouts`` (the CAPTURE / TIMEOUT planes' sums: episode ends counted at a
        valid position) and their argmax cells ``top_capture_cell`` / ``top_timeout_cell``.  Formed on the host from ``counts()``: one
        synchronisation."""
        c = self.counts()
        out = []
        for g in range(self.G):
            per_agent = {}
            for i, aid in enumerate(self.agents):
                occ, seen, spawn = c["counts"][g, OCC, i], c["counts"][g, SEEN, i], c["counts"][g, SPAWN, i]
                hidden = occ - seen
                n_occ = int(occ.sum())
                top = lambda plane: tuple(int(v) for v in np.unravel_index(int(plane.argmax()), plane.shape)) if plane.max() > 0 else None
                per_agent[aid] = {"outside": int(c["outside"][g, i]), "occupied": n_occ, "seen": int(seen.sum()), "spawns": int(spawn.sum()),
                                  "cells_visited": int((occ > 0).sum()), "seen_fraction": float(seen.sum()) / n_occ if n_occ else 0.0,
                                  "top_cell": top(occ), "top_hidden_cell": top(hidden)}
                if self.final_positions:
                    cap, tmo = c["ends"][g, CAPTURE, i], c["ends"][g, TIMEOUT, i]
                    per_agent[aid].update(captures=int(cap.sum()), timeouts=int(tmo.sum()), top_capture_cell=top(cap), top_timeout_cell=top(tmo))
            out.append({"rows": int(c["rows"][g]), "agents": per_agent})
        return out
