"""Shortest paths around the walls: a grid over each map, the all-pairs hop table on it, and the rule by which the PRIVILEGED yardstick
opponents ``"pursue"`` and ``"flee"`` (``selfplay/navigators.py``) move.  Privileged: they read ``team_positions`` and the map, which no
policy observes; they measure how far a cop or a thief is from one that knows the maze, and are no training target to imitate.

    field = NavField.from_env(env)                  # host tables per compiled map; on a GPU one launch of cat_render_nav_build
    action, hops = navigate_step(env.raw_outputs()["team_positions"], u, field, [0, 1], [0, 0], [0b100, 0b100])

This module IS the definition: ``free_cells`` / ``snap_cells`` / ``hops_reference`` (NumPy) of the tables and ``navigate_step`` (torch, any
device) of the tick.  ``cat_render_nav_build`` and ``cat_render_nav_step`` (include/cat_render.h) equal them exactly: every value is an
integer.

The grid of a map with window W x H: ``Wc = ceil(W / cell)``, ``Hc = ceil(H / cell)`` cells, cell (ix, iy) at index ``k = ix * Hc + iy``
(x-major, like ``positions.PositionTracker``), ``C = Wc * Hc <= MAX_CELLS``.

* ``free[k]``: the cell's centre ((ix + .5) cell, (iy + .5) cell) lies at least ``clearance`` inside the window on all four sides, outside
  every hull, and farther than ``clearance`` from every hull's boundary.  With ``clearance = agent_radius + wall_radius`` an agent's centre
  can stand there.
* ``snap[k]``: k for a free cell; for a blocked one the free cell with the smallest squared centre distance within Chebyshev distance 2
  (the lowest index on ties), ``NONE`` if there is none -- an agent in contact with a wall can stand in a cell whose centre is blocked.
* ``hops[goal][k]``: 4-connected steps over free cells, ``NONE`` where either is blocked or no path exists.

The tick, per row = (navigator g, env n) -- actions 0 = -x, 1 = +y, 2 = +x, 3 = -y as in ``selfplay/scripted.py``:

* the cell of a position (x, y) (f16): both finite, x >= 0, y >= 0, ix = int(floor(x)) // cell < Wc, iy = int(floor(y)) // cell < Hc, then
  ``snap[ix * Hc + iy]``; ``NONE`` is no cell.  a = the row's own cell, b_j the cells of its opponents j.
* target: among the opponents with a cell and ``hops[b_j][a] != NONE`` the smallest key ``(hops[b_j][a] << 8) | j``; d its hop count.
* fallback: no own cell, no target, or none of a's four neighbours usable (on the grid and free): ``min(3, int(4 u))``, ``nav_hops = -1``.
* pref: D = target position - own position (fp32); the x axis if |D.x| >= |D.y| else y; on x 2 if D.x >= 0 else 0, on y 1 if D.y >= 0 else 3.
* pursue: d == 0 -> pref.  Otherwise the usable neighbours with the smallest ``hops[b][nb_i]`` (one has d - 1): pref if it is one of them,
  else the lowest action.
* flee: per usable neighbour m_i = min and t_i = sum over ALL opponents with a cell of ``hops[b_j][nb_i]`` (``NONE`` counts as 65535: an
  unreachable threat is none): the largest m_i, then the largest t_i, then the lowest action.
* ``nav_hops`` = d: the geodesic separation of the row from its nearest opponent.

Potential-based reward shaping (Ng, Harada and Russell 1999) on the same table -- ``separation`` and ``shaping_step`` (torch, any device)
ARE its definition, and ``cat_render_nav_shape`` equals them bit for bit.  The learner's reward takes ``F = gamma Phi(s') - Phi(s)``, which
leaves the optimal policies as they are: over an episode the sum telescopes.

* ``separation(P, g)`` of agent g in a position array P (f16 [N, A, 2]), by the cell rule above: a = g's cell; d = the smallest
  ``hops[b_j][a]`` over the opponents j of ``opp_mask[g]`` that have a cell and whose entry is not ``NONE``; -1 if g has no cell or there
  is no such opponent.  (No neighbour needs to be usable: that is the navigators' concern.)
* ``phi(g, d) = coef[g] (*) float(min(d, cap))`` for d >= 0: one rounded fp32 multiply of an exactly converted integer.  ``coef[g]`` is
  negative for a cop (closer is better) and positive for a thief; ``cap`` is an integer in 1 .. 65534.
* One tick of row (g, n); its state ``hops_prev[g][n]`` (int32) is the separation at the start of the tick, d0:
  ``terminated[n]`` and not ``truncated[n]`` (a capture: a true terminal state): phi1 = +0.0, defined.
  ``terminated[n]`` and ``truncated[n]`` (the time limit, no property of the state): d1 = separation(final_positions, g).
  Otherwise d1 = separation(team_positions, g).
  F = +0.0 if d0 < 0 or a needed d1 < 0, else ``(gamma (*) phi1) (-) phi(g, d0)``: two rounded fp32 operations in that order, never fused.
  ``reward_out[g][n] = reward_out[g][n] (+) F`` (always performed), ``shaping_out[g][n] = F`` where given, and
  ``hops_prev[g][n] = separation(team_positions, g)`` -- always; on a terminal row that is the NEW episode's first state, because the env
  resets inside the tick.
* Prime mode: only the last assignment.
* ``final_positions`` is read on rows with ``terminated`` and ``truncated`` both set and nowhere else: every other row of it is stale or NaN.

A geodesic start-state curriculum on the same table -- ``spawn_step`` (torch, any device) IS its definition, and ``cat_render_nav_spawn``
equals it exactly: every output is an integer or an exactly representable f64.  It chooses start positions such that every cop stands a
chosen number of hops from a thief (``selfplay/curriculum.py`` hands them to the env core's masked reset).

* Slot n takes part iff ``mask[n] != 0`` and its band ``(lo, hi) = band[n]`` satisfies ``1 <= lo <= hi <= 65534``; any other band means
  "this slot keeps the map's own spawn".  Everything below is per participating slot, on its map ``slot_map[n]``.
* The draw among ``cnt`` candidates, visited in cell-index order: rank ``j = min(cnt - 1, int(u (*) float(cnt)))`` -- one rounded fp32
  multiply of an exactly converted integer, then truncation (``navigate_step``'s fallback has the same shape); u in [0, 1).
* Placement order: the thieves in env order, then the cops in env order; the i-th placed agent reads ``uniform[i][n]``.
  Thief 0 (the anchor): all free cells.  Every further thief: the free cells k with ``hops[anchor][k] != NONE`` that no earlier agent has
  taken.  Every cop: the free cells k not taken with ``lo <= d(k) <= hi``, ``d(k)`` the smallest ``hops[b_j][k]`` over the placed thieves'
  cells b_j, ``NONE`` entries ignored (all ``NONE``: no candidate).
* A placed agent stands at its cell's centre ((ix + .5) cell, (iy + .5) cell): exact in f64, exact in the f16 of ``team_positions`` on
  every map the field admits, farther than ``clearance`` from every wall by the definition of ``free``; distinct cells are ``cell`` = 16 px
  apart against two radii of 10, so agents never overlap.
* Fallback: an agent with ``cnt == 0`` gives ``placed[n] = 0`` and the slot's positions are NOT written (the env's own spawn stands); else
  ``placed[n] = 1``.  Rows that do not take part give ``placed[n] = 0`` and are not written.
* Nothing is checked about captures.  ``lo = 1`` puts a cop 16 px from a thief, inside the termination radius of 20, and the first tick
  captures; ``lo >= 2`` never does that (32 px straight, 22.6 px diagonal).
* The field must be the arena field (``NavField.from_env(env, arena=True)``), for the reason ``GeodesicShaper`` gives: on the plain field
  a free cell can lie outside the enclosure the agents play in.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_CELLS = 4096        # CAT_NAV_MAX_CELLS
MAX_MAPS = 16           # CAT_NAV_MAX_MAPS
NONE = 0xFFFF           # CAT_NAV_NONE
PURSUE, FLEE = 0, 1     # CAT_NAV_PURSUE / CAT_NAV_FLEE


def grid_shape(window, cell: int) -> Tuple[int, int]:
    """(Wc, Hc) of a window (W, H) at ``cell`` pixels per cell; ValueError above ``MAX_CELLS`` cells."""
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or cell < 1:
        raise ValueError(f"cell is the cell size in pixels, an integer >= 1, got {cell!r}")
    Wc, Hc = max(1, math.ceil(float(window[0]) / cell)), max(1, math.ceil(float(window[1]) / cell))
    if Wc * Hc > MAX_CELLS:
        raise ValueError(f"a {Wc} x {Hc} grid has more than {MAX_CELLS} cells: choose a larger cell than {cell}")
    return Wc, Hc


def hull_distance(cmap, points: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """For points float64 [P, 2]: (inside [P] -- inside or on some hull, by its planes; dist [P] -- the smallest Euclidean distance to any
    hull's boundary, +inf for a map without walls).  Hull vertices are ``planes[:, 2:4]``; edge i of a hull runs from vertex i - 1 to i."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    inside = np.zeros(len(pts), bool)
    dist = np.full(len(pts), np.inf)
    for first, count in zip(cmap.shape_first, cmap.shape_count):
        pl = cmap.planes[first:first + count]
        inside |= ((pts[:, 0:1] * pl[None, :, 0] + pts[:, 1:2] * pl[None, :, 1] - pl[None, :, 4]) <= 0.0).all(axis=1)
        b = pl[:, 2:4]
        a = np.roll(b, 1, axis=0)
        e = b - a                                                             # [k, 2]
        w = pts[:, None, :] - a[None]                                         # [P, k, 2]
        t = np.clip((w * e[None]).sum(-1) / (e * e).sum(-1)[None], 0.0, 1.0)
        q = w - t[..., None] * e[None]
        dist = np.minimum(dist, np.sqrt((q * q).sum(-1)).min(axis=1))
    return inside, dist


def free_cells(cmap, cell: int, clearance: float) -> Tuple[np.ndarray, int, int]:
    """(free uint8 [C], Wc, Hc) of one ``CompiledMap``: the rule of the module docstring."""
    W, H = float(cmap.window[0]), float(cmap.window[1])
    Wc, Hc = grid_shape((W, H), cell)
    cx = (np.repeat(np.arange(Wc), Hc) + 0.5) * cell
    cy = (np.tile(np.arange(Hc), Wc) + 0.5) * cell
    inside, dist = hull_distance(cmap, np.stack([cx, cy], axis=1))
    in_window = (cx >= clearance) & (cx <= W - clearance) & (cy >= clearance) & (cy <= H - clearance)
    return (in_window & ~inside & (dist > clearance)).astype(np.uint8), Wc, Hc


def snap_cells(free: np.ndarray, Wc: int, Hc: int) -> np.ndarray:
    """snap uint16 [C]: the rule of the module docstring."""
    f = np.asarray(free).reshape(Wc, Hc) != 0
    index = np.arange(Wc * Hc, dtype=np.int64).reshape(Wc, Hc)
    snap = np.where(f, index, NONE)
    todo = ~f
    # nearest first; among equally near cells the lowest index = the smallest dx, then the smallest dy
    offsets = sorted(((dx * dx + dy * dy, dx, dy) for dx in range(-2, 3) for dy in range(-2, 3) if (dx, dy) != (0, 0)))
    ix, iy = np.meshgrid(np.arange(Wc), np.arange(Hc), indexing="ij")
    for _, dx, dy in offsets:
        jx, jy = ix + dx, iy + dy
        ok = (jx >= 0) & (jx < Wc) & (jy >= 0) & (jy < Hc)
        hit = todo & ok & f[np.clip(jx, 0, Wc - 1), np.clip(jy, 0, Hc - 1)]
        snap[hit] = (jx * Hc + jy)[hit]
        todo &= ~hit
    return snap.reshape(-1).astype(np.uint16)


def hops_reference(free: np.ndarray, Wc: int, Hc: int, goals: Optional[Sequence[int]] = None) -> np.ndarray:
    """The all-pairs table uint16 [C, C] (or the rows ``goals``): ``hops[goal][k]`` = 4-connected breadth-first steps over free cells,
    ``NONE`` where goal or k is blocked or unreachable.

    Level-synchronous over boolean arrays, every goal at once: the booleans of one cell over all goals are packed eight to a byte (goal
    j = bit j % 8 of byte j // 8), so a level is a handful of byte-wise operations on [Wc, Hc, ceil(goals / 8)] arrays.  In level L every
    unvisited free cell with a 4-neighbour in the frontier takes L + 1, which is written bit by bit into 16 packed planes."""
    C = Wc * Hc
    f = np.asarray(free).reshape(Wc, Hc) != 0
    goals = np.arange(C) if goals is None else np.asarray(goals, dtype=np.int64).reshape(-1)
    n = len(goals)
    B = (n + 7) // 8
    front = np.zeros((Wc, Hc, B), np.uint8)
    j = np.arange(n)
    ok = f.reshape(-1)[goals]                                                 # a blocked goal reaches nothing: its row stays NONE
    np.bitwise_or.at(front, (goals[ok] // Hc, goals[ok] % Hc, j[ok] // 8), (1 << (j[ok] % 8)).astype(np.uint8))
    open_ = np.where(f, 0xFF, 0).astype(np.uint8)[:, :, None]
    visited = front.copy()
    planes = np.zeros((16, Wc, Hc, B), np.uint8)
    for level in range(1, C + 1):
        reach = np.zeros_like(front)
        reach[1:] |= front[:-1]
        reach[:-1] |= front[1:]
        reach[:, 1:] |= front[:, :-1]
        reach[:, :-1] |= front[:, 1:]
        front = reach & open_ & ~visited
        if not front.any():
            break
        visited |= front
        for p in range(16):
            if (level >> p) & 1:
                planes[p] |= front
    out = np.zeros((C, n), np.uint16)                                          # [cell, goal]
    for p in range(16):
        if planes[p].any():
            out |= np.unpackbits(planes[p].reshape(C, B), axis=1, bitorder="little")[:, :n].astype(np.uint16) << p
    out[np.unpackbits(visited.reshape(C, B), axis=1, bitorder="little")[:, :n] == 0] = NONE
    return np.ascontiguousarray(out.T)


def component_sizes(free: np.ndarray, Wc: int, Hc: int) -> List[int]:
    """Sizes of the 4-connected components of the free cells, largest first."""
    f = np.asarray(free).reshape(Wc, Hc) != 0
    label = np.where(f, np.arange(Wc * Hc).reshape(Wc, Hc), -1)
    while True:                                                                # every free cell takes the largest label it touches
        big = label.copy()
        big[1:] = np.maximum(big[1:], label[:-1]); big[:-1] = np.maximum(big[:-1], label[1:])
        big[:, 1:] = np.maximum(big[:, 1:], label[:, :-1]); big[:, :-1] = np.maximum(big[:, :-1], label[:, 1:])
        big = np.where(f, big, -1)
        if np.array_equal(big, label):
            break
        label = big
    return sorted((int(c) for c in np.bincount(label[f]) if c), reverse=True)


def arena_cells(cmap, cell: int, clearance: float) -> Tuple[np.ndarray, int, int]:
    """``free_cells`` restricted to the 4-connected components in which the map lets an agent start: those that hold the cell of a start
    position or of a spawn region's centre (``CompiledMap.start_pos``, ``.regions`` = x, y, w, h).  Everything else counts as blocked,
    so a blocked cell snaps INTO the arena.  Why: ``snap`` picks the nearest free cell without asking whether the agents can get there, and
    a wall thinner than a cell has free cells on both sides at the same distance -- on squarinth an agent that touches the top or the left
    wall from inside would snap to the ground outside the enclosure and lose every separation.  (All of a map's free cells are kept where
    none of these points lies in a free cell.)"""
    free, Wc, Hc = free_cells(cmap, cell, clearance)
    pts = [np.asarray(cmap.start_pos, np.float64).reshape(-1, 2)]
    reg = np.asarray(cmap.regions, np.float64).reshape(-1, 4)
    pts.append(reg[:, :2] + 0.5 * reg[:, 2:])
    pts = np.concatenate(pts)
    ix, iy = np.floor(pts[:, 0]).astype(np.int64) // cell, np.floor(pts[:, 1]).astype(np.int64) // cell
    on = (pts >= 0).all(axis=1) & (ix < Wc) & (iy < Hc)
    seeds = np.unique((ix * Hc + iy)[on])
    seeds = seeds[free[seeds] != 0]
    if not len(seeds):
        return free, Wc, Hc
    reached = (hops_reference(free, Wc, Hc, goals=seeds) != NONE).any(axis=0)
    return (free * reached).astype(np.uint8), Wc, Hc


class NavField:
    """The tables of a batch of maps, on ``device``.

    ``cell``; ``grid_host`` int32 NumPy [M, 4] = (Wc, Hc, cell_off, hops_off): map m's first element in ``free`` / ``snap`` and in
    ``hops``; ``grid`` the same as a tensor; ``free`` uint8 [sum C]; ``snap`` and ``hops`` [sum C] / [sum C^2] hold uint16 values in
    int16 tensors (``& 0xFFFF`` after widening; ``NONE`` reads -1); ``slot_map`` int32 [N].  ``free_of`` / ``snap_of`` / ``hops_of`` give
    one map's tables as NumPy arrays in their own types."""

    def __init__(self, cell: int, masks: Sequence[Tuple[np.ndarray, int, int]], slot_map, device="cpu"):
        """``masks``: per map (free uint8 [C], Wc, Hc).  On a GPU the hop table is built there by ``cat_render_nav_build`` (a missing
        kernel is an error), elsewhere by ``hops_reference``."""
        if not 1 <= len(masks) <= MAX_MAPS:
            raise ValueError(f"a field has 1 .. {MAX_MAPS} maps, not {len(masks)}")
        if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or cell < 1:
            raise ValueError(f"cell is the cell size in pixels, an integer >= 1, got {cell!r}")
        self.cell, self.device = int(cell), torch.device(device)
        rows, cells, entries = [], 0, 0
        for free, Wc, Hc in masks:
            C = int(Wc) * int(Hc)
            if Wc < 1 or Hc < 1 or C > MAX_CELLS or np.asarray(free).size != C:
                raise ValueError(f"a grid of {Wc} x {Hc} cells with a mask of {np.asarray(free).size}: 1 .. {MAX_CELLS} cells, one mask entry each")
            rows.append((Wc, Hc, cells, entries))
            cells, entries = cells + C, entries + C * C
        self.grid_host = np.array(rows, dtype=np.int32).reshape(len(masks), 4)
        free_all = np.concatenate([(np.asarray(f).reshape(-1) != 0).astype(np.uint8) for f, _, _ in masks])
        snap_all = np.concatenate([snap_cells(f, Wc, Hc) for f, Wc, Hc in masks])
        slot_map = np.asarray(slot_map, dtype=np.int32).reshape(-1)
        if slot_map.size and (slot_map.min() < 0 or slot_map.max() >= len(masks)):
            raise ValueError(f"slot_map names a map outside [0, {len(masks)})")
        self.grid = torch.from_numpy(self.grid_host.copy()).to(self.device)
        self.free = torch.from_numpy(free_all).to(self.device)
        self.snap = torch.from_numpy(snap_all.view(np.int16).copy()).to(self.device)
        self.slot_map = torch.from_numpy(slot_map.copy()).to(self.device)
        if self.device.type == "cuda":
            from . import _learn_native
            self.hops = torch.empty(entries, dtype=torch.int16, device=self.device)
            with torch.cuda.device(self.device):
                _learn_native.nav_build(self.grid_host, self.grid, self.free, self.hops)
        else:
            self.hops = torch.from_numpy(np.concatenate([hops_reference(f, Wc, Hc).reshape(-1) for f, Wc, Hc in masks]).view(np.int16).copy())

    @classmethod
    def from_maps(cls, compiled, slot_map, cell: int = 16, clearance: float = 6.0, device="cpu", arena: bool = False) -> "NavField":
        """The field of ``CompiledMap``s: ``free_cells`` of each, or with ``arena`` its ``arena_cells``."""
        return cls(cell, [(arena_cells if arena else free_cells)(cm, cell, clearance) for cm in compiled], slot_map, device)

    @classmethod
    def from_env(cls, env, cell: int = 16, clearance: Optional[float] = None, arena: bool = False) -> "NavField":
        """The field of ``env``'s compiled maps and slots; ``clearance`` defaults to the env's agent_radius + wall_radius (6.0 with the
        default physics); ``arena``: ``arena_cells`` instead of ``free_cells``."""
        cfg = env._cfg
        if clearance is None:
            clearance = float(cfg.agent_radius) + float(cfg.wall_radius)
        slot_map = getattr(env, "slot_map_ids", None)
        if slot_map is None:
            slot_map = np.zeros(env.num_envs, dtype=np.int32)
        return cls.from_maps(env._compiled, slot_map, cell, float(clearance), env.device, **({"arena": True} if arena else {}))

    @property
    def n_maps(self) -> int:
        return self.grid_host.shape[0]

    def _cells(self, m: int) -> Tuple[int, int, int, int]:
        Wc, Hc, off, hoff = (int(v) for v in self.grid_host[m])
        return Wc * Hc, off, hoff, Hc

    def free_of(self, m: int) -> np.ndarray:
        C, off, _, _ = self._cells(m)
        return self.free[off:off + C].cpu().numpy()

    def snap_of(self, m: int) -> np.ndarray:
        C, off, _, _ = self._cells(m)
        return self.snap[off:off + C].cpu().numpy().view(np.uint16)

    def hops_of(self, m: int) -> np.ndarray:
        C, _, hoff, _ = self._cells(m)
        return self.hops[hoff:hoff + C * C].cpu().numpy().view(np.uint16).reshape(C, C)

    def component_sizes(self) -> List[List[int]]:
        """Per map the sizes of the connected components of its free cells, largest first."""
        return [component_sizes(self.free_of(m), int(self.grid_host[m, 0]), int(self.grid_host[m, 1])) for m in range(self.n_maps)]


def _cells_and_hops(positions: torch.Tensor, field: NavField):
    """The cell and hop lookup that ``navigate_step`` and ``separation`` share, for positions f16 [N, A, 2]: (pos fp32 [N, A, 2], cells
    int64 [N, A] -- every agent's snapped cell by the rule of the module docstring, -1 = none --, H, (Wc, Hc, coff, free)) with
    ``H(b, k)`` = ``hops[b][k]`` of the row's map where both are cells and ``NONE`` elsewhere (b, k int64 [N, ...]), Wc / Hc / coff [N, 1]
    the row's grid and its first element in the per-cell arrays, ``free`` the field's mask on the positions' device."""
    N = positions.shape[0]
    assert positions.dtype == torch.float16 and positions.dim() == 3 and positions.shape[2] == 2
    dev, i64 = positions.device, torch.int64
    cell, M = field.cell, field.n_maps
    pos = positions.float()                                                    # f16 -> fp32 is exact
    bits = positions.view(torch.int16).to(i64) & 0xFFFF
    finite = ((bits & 0x7C00) != 0x7C00).all(-1)
    m = field.slot_map.to(dev).to(i64)
    map_ok = (m >= 0) & (m < M)
    row = field.grid.to(dev).to(i64)[m.clamp(0, M - 1)]                        # [N, 4]
    Wc, Hc, coff, hoff = (row[:, c].unsqueeze(1) for c in range(4))            # [N, 1]
    C = Wc * Hc
    free, snap, hops = field.free.to(dev), field.snap.to(dev), field.hops.to(dev)

    valid = finite & (pos[..., 0] >= 0) & (pos[..., 1] >= 0) & map_ok.unsqueeze(1)
    safe = torch.where(valid.unsqueeze(-1), pos, torch.zeros_like(pos))
    ix, iy = safe[..., 0].floor().to(i64) // cell, safe[..., 1].floor().to(i64) // cell
    valid = valid & (ix < Wc) & (iy < Hc)
    s = snap[coff + torch.where(valid, ix * Hc + iy, torch.zeros_like(ix))].to(i64) & 0xFFFF
    cells = torch.where(valid & (s < C), s, torch.full_like(s, -1))            # [N, A]: the cell of every agent, -1 = none

    def H(b, k):                                                               # hops[b][k] where both are cells, NONE elsewhere
        ok = (b >= 0) & (k >= 0)
        per_row = (N,) + (1,) * (ok.dim() - 1)
        v = hops[hoff.view(per_row) + torch.where(ok, b * C.view(per_row) + k, torch.zeros_like(b + k))].to(i64) & 0xFFFF
        return torch.where(ok, v, torch.full_like(v, NONE))

    return pos, cells, H, (Wc, Hc, coff, free)


@torch.no_grad()
def navigate_step(team_positions: torch.Tensor, uniform: torch.Tensor, field: NavField, agent_index: Sequence[int], script,
                  opponent_mask: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rule of the module docstring: team_positions f16 [N, A, 2], uniform fp32 [G, N], per navigator g its env agent index, its
    script (an int or an integer tensor [N] per navigator, or one tensor [G, N]: PURSUE, FLEE or -1) and the bitmask of its opponents'
    agent indices.  Returns (action int32 [G, N], nav_hops int32 [G, N]); both are -1 where the script is -1, and nav_hops is -1 after
    the fallback.  Nothing is modified."""
    N, A, _ = team_positions.shape
    G = len(agent_index)
    assert team_positions.dtype == torch.float16 and uniform.dtype == torch.float32 and tuple(uniform.shape) == (G, N)
    dev, i64 = team_positions.device, torch.int64
    pos, cells, H, (Wc, Hc, coff, free) = _cells_and_hops(team_positions, field)

    script_t = torch.stack([torch.as_tensor(sc, device=dev).to(i64).expand(N) for sc in script]) if not torch.is_tensor(script) else \
        script.to(dev).to(i64).expand(G, N)
    actions, nav = [], []
    four = torch.arange(4, device=dev)
    big = 1 << 40
    for g in range(G):
        me, opp = int(agent_index[g]), [j for j in range(A) if (int(opponent_mask[g]) >> j) & 1]
        a = cells[:, me:me + 1]                                                # [N, 1]
        u = uniform[g]
        fallback = (4.0 * u).to(i64).clamp(max=3)
        if not opp:
            actions.append(fallback); nav.append(torch.full_like(fallback, -1))
            continue
        opp_t = torch.tensor(opp, device=dev)
        b = cells[:, opp_t]                                                    # [N, J]
        ha = H(b, a)
        key = torch.where(ha != NONE, (ha << 8) | opp_t, torch.full_like(ha, big))
        best, arg = key.min(dim=1)                                             # (keys are distinct: the first minimum is the only one)
        has = best < big
        d = best >> 8
        bt = torch.where(has, b.gather(1, arg.unsqueeze(1)).squeeze(1), torch.full_like(d, -1)).unsqueeze(1)
        delta = pos[:, opp_t].gather(1, arg.view(N, 1, 1).expand(N, 1, 2)).squeeze(1) - pos[:, me]
        dx, dy = delta[:, 0], delta[:, 1]
        pref = torch.where(dx.abs() >= dy.abs(), torch.where(dx >= 0, 2, 0), torch.where(dy >= 0, 1, 3))
        # the four neighbours by action
        a0 = a.clamp(min=0)
        aix, aiy = a0 // Hc, a0 % Hc
        nb = torch.cat([a0 - Hc, a0 + 1, a0 + Hc, a0 - 1], dim=1)               # [N, 4]
        on = torch.cat([aix > 0, aiy + 1 < Hc, aix + 1 < Wc, aiy > 0], dim=1) & (a >= 0)
        use = on & (free[coff + torch.where(on, nb, torch.zeros_like(nb))] != 0)
        nbu = torch.where(use, nb, torch.full_like(nb, -1))
        # pursue
        v = torch.where(use, H(bt.expand(N, 4), nbu), torch.full_like(nb, big))
        at_min = v == v.min(dim=1, keepdim=True).values
        lowest = torch.where(at_min, four, 4).min(dim=1).values
        chase = torch.where(at_min.gather(1, pref.unsqueeze(1)).squeeze(1), pref, lowest)
        chase = torch.where(d == 0, pref, chase)
        # flee
        h = H(b.unsqueeze(2).expand(N, len(opp), 4), nbu.unsqueeze(1).expand(N, len(opp), 4))        # [N, J, 4]; NONE where b has no cell
        has_cell = (b >= 0).unsqueeze(2)
        lo = h.min(dim=1).values
        total = torch.where(has_cell, h, torch.zeros_like(h)).sum(dim=1)
        score = torch.where(use, (lo << 32) | total, torch.full_like(lo, -1))
        away = torch.where(score == score.max(dim=1, keepdim=True).values, four, 4).min(dim=1).values
        ok = (a.squeeze(1) >= 0) & has & use.any(dim=1)
        sc = script_t[g]
        act = torch.where(ok, torch.where(sc == FLEE, away, chase), fallback)
        actions.append(torch.where(sc >= 0, act, torch.full_like(act, -1)))
        nav.append(torch.where((sc >= 0) & ok, d, torch.full_like(d, -1)))
    return torch.stack(actions).to(torch.int32), torch.stack(nav).to(torch.int32)


@torch.no_grad()
def separation(positions: torch.Tensor, field: NavField, agent_index: Sequence[int], opponent_mask: Sequence[int]) -> torch.Tensor:
    """The geodesic separation int32 [G, N] of the module docstring for positions f16 [N, A, 2]: per row (g, n) the smallest
    ``hops[b_j][a]`` over g's opponents with a cell and an entry that is not ``NONE``; -1 where g has no cell or there is no such opponent."""
    N, A, _ = positions.shape
    _, cells, H, _ = _cells_and_hops(positions, field)
    out = []
    for g in range(len(agent_index)):
        me, opp = int(agent_index[g]), [j for j in range(A) if (int(opponent_mask[g]) >> j) & 1]
        if not opp:
            out.append(torch.full((N,), -1, dtype=torch.int64, device=positions.device))
            continue
        d = H(cells[:, opp], cells[:, me:me + 1]).min(dim=1).values            # NONE where either has no cell: the largest value
        out.append(torch.where(d != NONE, d, torch.full_like(d, -1)))
    return torch.stack(out).to(torch.int32)


@torch.no_grad()
def shaping_step(team_positions: torch.Tensor, final_positions: Optional[torch.Tensor], terminated: Optional[torch.Tensor],
                 truncated: Optional[torch.Tensor], field: NavField, agent_index: Sequence[int], opponent_mask: Sequence[int],
                 coef: Sequence[float], gamma: float, cap: int, hops_prev: torch.Tensor, reward_out: Optional[torch.Tensor] = None,
                 shaping_out: Optional[torch.Tensor] = None, prime: bool = False) -> None:
    """One tick of the shaping rule of the module docstring, in place: team_positions / final_positions f16 [N, A, 2], terminated /
    truncated [N] (bool or u8), per shaped agent g its env agent index, the bitmask of its opponents and its fp32 coefficient; ``gamma``
    is rounded to fp32 once.  ``hops_prev`` int32 [G, N] is read and rewritten, ``reward_out`` fp32 [G, N] (any row stride) takes
    ``(+) F`` and ``shaping_out`` (where given) ``F``.  ``prime``: only ``hops_prev`` is written, and only team_positions is read."""
    N, A, _ = team_positions.shape
    G = len(agent_index)
    if not (isinstance(cap, (int, np.integer)) and not isinstance(cap, bool) and 1 <= cap <= 65534):
        raise ValueError(f"cap is a hop count in 1 .. 65534, got {cap!r}")
    assert hops_prev.dtype == torch.int32 and tuple(hops_prev.shape) == (G, N) and len(opponent_mask) == G == len(coef)
    d_now = separation(team_positions, field, agent_index, opponent_mask)
    if not prime:
        dev, f32 = team_positions.device, torch.float32
        assert reward_out is not None and reward_out.dtype == f32 and tuple(reward_out.shape) == (G, N)
        assert shaping_out is None or (shaping_out.dtype == f32 and tuple(shaping_out.shape) == (G, N))
        term, trunc = (terminated.to(dev) != 0).view(1, N), (truncated.to(dev) != 0).view(1, N)
        capture, timeout = term & ~trunc, term & trunc
        d_fin = separation(final_positions, field, agent_index, opponent_mask)   # (rows that are no timeout drop out in the next line)
        d0, d1 = hops_prev.to(dev), torch.where(timeout, d_fin, d_now)
        c = torch.tensor([float(v) for v in coef], dtype=f32, device=dev).view(G, 1)
        g32 = torch.tensor(float(gamma), dtype=f32, device=dev)
        phi = lambda d: c * d.clamp(0, int(cap)).to(f32)                       # one rounded multiply; the conversion is exact
        zero = torch.zeros(G, N, dtype=f32, device=dev)
        phi1 = torch.where(capture, zero, phi(d1))
        F = torch.where((d0 >= 0) & (capture | (d1 >= 0)), g32 * phi1 - phi(d0), zero)    # two rounded operations, in this order
        reward_out.copy_(reward_out + F)
        if shaping_out is not None:
            shaping_out.copy_(F)
    hops_prev.copy_(d_now)


BAND_MAX = 65534        # the largest hop count a band may name (NONE - 1)


@torch.no_grad()
def spawn_step(mask: torch.Tensor, uniform: torch.Tensor, band: torch.Tensor, field: NavField, n_cops: int,
               positions: Optional[torch.Tensor] = None, placed: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The start-state rule of the module docstring: mask u8 / bool [N], uniform fp32 [A, N], band int32 [N, 2], ``n_cops`` in 1 .. A - 1
    (env order: cops first).  Returns (positions f64 [N, A, 2], placed u8 [N]).  ``positions`` / ``placed``, where given, are written in
    place: ``placed`` in every row, ``positions`` in the rows with ``placed[n] == 1`` and in no other (fresh ones are zero there)."""
    A, N = uniform.shape
    if not (isinstance(n_cops, (int, np.integer)) and not isinstance(n_cops, bool) and 1 <= n_cops <= A - 1):
        raise ValueError(f"n_cops must lie in 1 .. A - 1 = {A - 1}, got {n_cops!r}")
    assert uniform.dtype == torch.float32 and tuple(mask.shape) == (N,) and tuple(band.shape) == (N, 2) and band.dtype == torch.int32
    dev, i64 = uniform.device, torch.int64
    nt = A - int(n_cops)
    row = field.grid.to(dev).to(i64)[field.slot_map.to(dev).to(i64)]                     # [N, 4]
    Wc, Hc, coff, hoff = (row[:, c].unsqueeze(1) for c in range(4))            # [N, 1]
    C = Wc * Hc
    k = torch.arange(int(C.max()) if N else 1, device=dev).view(1, -1)         # every map's cells, padded to the largest grid
    on = k < C
    k0 = torch.where(on, k, torch.zeros_like(k))
    free = on & (field.free.to(dev)[coff + k0] != 0)                           # [N, K]
    hops = field.hops.to(dev)
    rows = torch.arange(N, device=dev)

    def hop_row(b):                                                            # hops[b][k] of the row's map, NONE off its grid
        v = hops[hoff + b.view(N, 1) * C + k0].to(i64) & 0xFFFF
        return torch.where(on, v, torch.full_like(v, NONE))

    lo, hi = band[:, 0:1].to(dev).to(i64), band[:, 1:2].to(dev).to(i64)
    ok = (mask.to(dev) != 0) & ((lo >= 1) & (lo <= hi) & (hi <= BAND_MAX)).squeeze(1)
    taken = torch.zeros_like(free)
    d = torch.full(free.shape, NONE, dtype=i64, device=dev)                    # the smallest hop count to a placed thief
    reach, picks = None, []
    for i in range(A):
        if i == 0:
            cand = free
        elif i < nt:
            cand = free & ~taken & (reach != NONE)
        else:
            cand = free & ~taken & (d != NONE) & (d >= lo) & (d <= hi)
        cnt = cand.sum(dim=1)
        j = torch.minimum((uniform[i] * cnt.to(torch.float32)).to(i64).clamp(min=0), cnt - 1)       # one rounded multiply, truncated
        ok = ok & (cnt > 0)
        pick = (cand & (cand.cumsum(dim=1) == (j + 1).view(N, 1))).to(torch.uint8).argmax(dim=1)     # the j-th candidate in cell order
        picks.append(pick)
        taken = taken.clone()
        taken[rows, pick] = True
        if i < nt:
            r = hop_row(pick)
            reach = r if i == 0 else reach
            d = torch.minimum(d, r)
    if positions is None:
        positions = torch.zeros(N, A, 2, dtype=torch.float64, device=dev)
    if placed is None:
        placed = torch.zeros(N, dtype=torch.uint8, device=dev)
    assert positions.dtype == torch.float64 and tuple(positions.shape) == (N, A, 2) and placed.dtype == torch.uint8 and tuple(placed.shape) == (N,)
    order = list(range(int(n_cops), A)) + list(range(int(n_cops)))             # the env column of the i-th placed agent
    cells = torch.stack(picks, dim=1)                                          # [N, A] in placement order
    centre = torch.stack([cells // Hc, cells % Hc], dim=2).to(torch.float64).add(0.5).mul(float(field.cell))
    new = positions.clone()
    new[:, order] = centre.to(positions.device)
    positions.copy_(torch.where(ok.view(N, 1, 1).to(positions.device), new, positions))
    placed.copy_(ok.to(torch.uint8))
    return positions, placed
