"""A geometric ground truth for the ray sensor, the capture predicate and the spawn rule, in NumPy float64.

Written from the geometry, not from Chipmunk's functions and not from the kernels: a wall is the set of points within
``wall_radius`` of a convex polygon, a ray is a disc of ``ray_radius`` swept along a segment, and the first contact is the
smallest parameter at which the disc's centre is exactly ``rho = wall_radius + ray_radius`` away from the polygon.  Candidate
parameters come from every vertex circle and every offset edge line; the DISTANCE FUNCTION decides which of them lie on the
offset outline, so there is no edge / corner case analysis of the kind ``poly_segment_query`` does.  The hull is gift-wrapped
(the product sorts and chains, the oracle restates QuickHull).

This module imports nothing from ``oracle`` and nothing from the product: maps arrive as plain data (the ``spec`` a compiled map
carries: the parsed JSON and the override arguments), configurations as plain numbers, states as arrays.

The only Chipmunk conventions modelled are the ones a geometric argument cannot replace: a shape counts only if the thin segment
enters its bounding box (``tbb``: where), and a query whose start lies within the radius reports the segment END as its point.
Whatever depends on the visiting order of the shapes is not predicted, and neither is a decision within ``DELTA`` of its threshold:
a start distance against ``rho``, a box entry or an alpha against 1, a hit against a miss (a graze; a box touched at a corner), a
coordinate of the reported point against a float16 rounding tie.  Such rays are "not clear": they are counted, not compared.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

WALL, COP, THIEF, MOVABLE, EMPTY = range(5)
DELTA = 1e-6            # margin of the clear rule: parameters (alpha, tbb) and origin distances (px)
ON_OUTLINE = 1e-7       # a root counts if the distance function puts it this close to the offset outline (px)
PREDICATE_MARGIN = 1e-9  # capture / spawn thresholds (px)
GOLDEN_MAPS = Path(__file__).resolve().parent / "golden" / "reference_maps.json"


# ---- maps as plain data --------------------------------------------------------------------------------------------------------
def _ring(block: dict):
    """One block of the reference's map schema -> its vertex list (rect: x, y and w, h defaulting to 1; poly: ``vs``)."""
    if block.get("type", "rect") == "rect":
        x, y = float(block["x"]), float(block["y"])
        w = 1.0 if block.get("w") is None else float(block["w"])
        h = 1.0 if block.get("h") is None else float(block["h"])
        return [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    return [(float(v["x"]), float(v["y"])) for v in block["vs"]]


def gift_wrap(points) -> np.ndarray:
    """Convex hull by Jarvis' march: from the lowest-leftmost point, the next vertex is the one that leaves every other point on its
    left; among points in line with it the farthest wins, so collinear and repeated points drop out.  -> [k, 2], counter-clockwise."""
    pts = np.unique(np.asarray(points, np.float64), axis=0)          # sorted by x, then y
    scale = max(1.0, float(np.abs(pts).max()))
    hull = [0]
    while True:
        cur = pts[hull[-1]]
        nxt = -1
        for q in range(len(pts)):
            if q == hull[-1]:
                continue
            if nxt < 0:
                nxt = q
                continue
            a, b = pts[nxt] - cur, pts[q] - cur
            turn = a[0] * b[1] - a[1] * b[0]
            if turn < -1e-12 * scale * scale or (abs(turn) <= 1e-12 * scale * scale and b @ b > a @ a):
                nxt = q                                                # q lies to the right of cur -> nxt (or beyond it on the same line)
        if nxt == hull[0]:
            break
        hull.append(nxt)
        assert len(hull) <= len(pts), "gift wrapping did not close"
    return pts[hull]


def map_hulls(spec: dict):
    """The convex hull of every wall ring of a map, from the map's plain data.  The five bundled maps are read from the reference's
    own files (tests/golden/reference_maps.json); any other map from the JSON it was loaded from."""
    data = spec["map_data"]
    if spec.get("bundled"):
        data = json.loads(GOLDEN_MAPS.read_text())["maps"][spec["name"]]
    sx, sy = spec.get("scale") or (1.0, 1.0)
    return [gift_wrap([(x * sx, y * sy) for x, y in _ring(b)]) for b in data["objects"]["blocks"]]


def agent_tables(spec: dict):
    """-> (start positions [A, 2], spawn regions per agent: a list of (x, y, w, h)), cops first, then thieves."""
    if spec.get("roster") is not None:
        agents = [{"type": t, "x": p[0], "y": p[1]} for t, p in zip(spec["roster"], spec["start_positions"])]
    else:
        data = spec["map_data"]
        if spec.get("bundled"):
            data = json.loads(GOLDEN_MAPS.read_text())["maps"][spec["name"]]
        agents = data["agents"]
    rows, seen = [], {}
    for a in agents:
        k = seen.get(a["type"], 0)
        seen[a["type"]] = k + 1
        regs = a.get("spawn_regions", a.get("spawn_region"))
        regs = [regs] if isinstance(regs, dict) else (regs or [])
        regs = (spec.get("spawn_regions") or {}).get(f"{a['type']}_{k}", regs)
        rows.append((a["type"], (float(a["x"]), float(a["y"])), [(float(r["x"]), float(r["y"]), float(r["w"]), float(r["h"])) for r in regs]))
    rows = [r for r in rows if r[0] == "cop"] + [r for r in rows if r[0] == "thief"]
    return np.array([r[1] for r in rows]), [r[2] for r in rows]


# ---- distances -----------------------------------------------------------------------------------------------------------------
def _edges(V):
    A = np.asarray(V, np.float64)
    return A, np.roll(A, -1, axis=0)


def _outward_normals(V):
    A, B = _edges(V)
    E = B - A
    area2 = float(np.sum(A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0]))
    n = np.stack([E[:, 1], -E[:, 0]], 1) * (1.0 if area2 > 0 else -1.0)
    return n / np.hypot(n[:, 0], n[:, 1])[:, None]


def hull_distance(V, p):
    """Distance from the points ``p`` [m, 2] (or one point) to the convex polygon ``V`` [k, 2], 0 inside, and the closest points."""
    P = np.atleast_2d(np.asarray(p, np.float64))
    A, B = _edges(V)
    E = B - A
    W = P[:, None, :] - A[None]
    t = np.clip(np.einsum("mkc,kc->mk", W, E) / np.einsum("kc,kc->k", E, E), 0.0, 1.0)
    C = A[None] + t[..., None] * E[None]
    dist = np.hypot(P[:, None, 0] - C[..., 0], P[:, None, 1] - C[..., 1])
    j = np.argmin(dist, axis=1)
    turn = E[None, :, 0] * W[..., 1] - E[None, :, 1] * W[..., 0]
    inside = np.all(turn >= 0.0, axis=1) | np.all(turn <= 0.0, axis=1)
    rows = np.arange(len(P))
    d = np.where(inside, 0.0, dist[rows, j])
    c = np.where(inside[:, None], P, C[rows, j])
    if np.ndim(p) == 1:
        return float(d[0]), c[0]
    return d, c


def _point_segment_distance(Q, P0, P1):
    """Distance from each point of ``Q`` [k, 2] to each segment ``P0[i] -> P1[i]`` [m, 2] -> [m, k]."""
    D = P1 - P0
    dd = np.einsum("mc,mc->m", D, D)
    W = Q[None] - P0[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dd[:, None] > 0.0, np.einsum("mkc,mc->mk", W, D) / dd[:, None], 0.0)
    t = np.clip(t, 0.0, 1.0)
    C = P0[:, None, :] + t[..., None] * D[:, None, :]
    return np.hypot(Q[None, :, 0] - C[..., 0], Q[None, :, 1] - C[..., 1])


def segment_hull_distance(V, P0, P1):
    """Distance between the segments ``P0[i] -> P1[i]`` and the convex polygon ``V``: 0 where they meet.  The part of a segment
    inside the polygon is what every edge's half-plane leaves of it; when nothing is left, two convex sets that do not meet are
    closest at a vertex of one of them: an end of the segment, or a vertex of the polygon."""
    P0, P1 = np.atleast_2d(np.asarray(P0, np.float64)), np.atleast_2d(np.asarray(P1, np.float64))
    A, _ = _edges(V)
    n = _outward_normals(V)
    s0 = np.einsum("mkc,kc->mk", P0[:, None, :] - A[None], n)
    s1 = np.einsum("mkc,kc->mk", P1[:, None, :] - A[None], n)
    ds = s1 - s0
    with np.errstate(divide="ignore", invalid="ignore"):
        cut = -s0 / ds
    lo = np.max(np.where(ds < 0.0, cut, 0.0), axis=1)
    hi = np.min(np.where(ds > 0.0, cut, 1.0), axis=1)
    out_all_along = np.any((ds == 0.0) & (s0 > 0.0), axis=1)
    meets = (lo <= hi) & ~out_all_along
    apart = np.minimum(np.minimum(hull_distance(V, P0)[0], hull_distance(V, P1)[0]), _point_segment_distance(A, P0, P1).min(axis=1))
    return np.where(meets, 0.0, apart)


# ---- first contact ---------------------------------------------------------------------------------------------------------------
def wall_alpha(V, rho, o, d):
    """First contact of a point moving ``o -> o + d`` with the outline at distance ``rho`` around the convex polygon ``V``.
    -> (alpha, marginal): alpha is 0 where the start is within ``rho``, the smallest entering root on the outline in [0, 1],
    or inf; marginal where the start distance, the alpha, or the hit / miss decision itself sits within DELTA of its threshold."""
    O, D = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
    A, _ = _edges(V)
    n = _outward_normals(V)
    d0 = hull_distance(V, O)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        # vertex circles |o + t d - v| = rho: the smaller root is where the circle is entered
        W = O[:, None, :] - A[None]
        a = np.einsum("mc,mc->m", D, D)[:, None]
        b = np.einsum("mkc,mc->mk", W, D)
        c = np.einsum("mkc,mkc->mk", W, W) - rho * rho
        disc = b * b - a * c
        t_circle = np.where(disc >= 0.0, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, np.inf)
        # edge lines pushed out by rho, n . (p - v) = rho: entered where the motion runs against the outward normal
        dn = D @ n.T
        t_line = np.where(dn < 0.0, (rho - np.einsum("mkc,kc->mk", W, n)) / dn, np.inf)
    T = np.concatenate([t_circle, t_line], axis=1)
    T = np.where(np.isfinite(T) & (T >= 0.0) & (T <= 1.0 + DELTA), T, np.inf)
    rows, cols = np.nonzero(np.isfinite(T))
    if len(rows):
        pts = O[rows] + T[rows, cols][:, None] * D[rows]
        off = np.abs(hull_distance(V, pts)[0] - rho) < ON_OUTLINE
        T[rows[~off], cols[~off]] = np.inf
    alpha = np.where(d0 <= rho, 0.0, T.min(axis=1))
    marginal = (np.abs(d0 - rho) < DELTA) | (np.abs(alpha - 1.0) < DELTA) | \
               ((d0 > rho) & (np.abs(segment_hull_distance(V, O, O + D) - rho) < DELTA))
    return np.where(alpha < 1.0, alpha, np.inf), marginal


def disc_alpha(C, rho, O, D):
    """The same for a disc of radius ``rho`` about the centres ``C`` [m, 2] (one per ray)."""
    W = O - C
    d0 = np.hypot(W[:, 0], W[:, 1])
    a = np.einsum("mc,mc->m", D, D)
    b = np.einsum("mc,mc->m", W, D)
    disc = b * b - a * (d0 * d0 - rho * rho)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(disc >= 0.0, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, np.inf)
    t = np.where((t >= 0.0) & (t <= 1.0 + DELTA), t, np.inf)
    alpha = np.where(d0 <= rho, 0.0, t)
    nearest = _point_segment_distance(np.zeros((1, 2)), W, W + D)[:, 0]      # distance from the centre to the segment
    marginal = (np.abs(d0 - rho) < DELTA) | (np.abs(alpha - 1.0) < DELTA) | ((d0 > rho) & (np.abs(nearest - rho) < DELTA))
    return np.where(alpha < 1.0, alpha, np.inf), marginal


def box_entry(bb, O, D):
    """Where the thin segment ``O -> O + D`` enters the box ``bb`` (l, b, r, t; [4] or one per ray), clamped to 0; inf if it does
    not meet the box within the segment."""
    bb = np.broadcast_to(np.asarray(bb, np.float64), (len(O), 4))
    lo, hi = bb[:, 0:2], bb[:, 2:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - O) / D, (hi - O) / D
    t_in, t_out = np.minimum(t1, t2), np.maximum(t1, t2)
    still, between = D == 0.0, (lo <= O) & (O <= hi)
    t_in = np.where(still, np.where(between, -np.inf, np.inf), t_in)
    t_out = np.where(still, np.where(between, np.inf, -np.inf), t_out)
    enter, leave = t_in.max(axis=1), t_out.min(axis=1)
    return np.where((enter <= leave) & (leave >= 0.0) & (enter <= 1.0), np.maximum(enter, 0.0), np.inf)


def gate(bb, O, D):
    """-> (tbb, marginal): marginal where the decision ``tbb < 1`` changes when the box grows or shrinks by DELTA."""
    bb = np.asarray(bb, np.float64)
    grow = np.array([-DELTA, -DELTA, DELTA, DELTA])
    tbb = box_entry(bb, O, D)
    marginal = ((box_entry(bb + grow, O, D) < 1.0) != (box_entry(bb - grow, O, D) < 1.0)) | (np.abs(tbb - 1.0) < DELTA)
    return tbb, marginal


def f16_tie(X):
    """Is a coordinate within PREDICATE_MARGIN of the midpoint of two neighbouring float16 values?  Rounding it to float16 is a
    decision like any other: two float64 evaluations of one point, 1e-13 apart, land on different sides of such a midpoint."""
    X = np.asarray(X, np.float64)
    h = X.astype(np.float16)
    mids = [(h.astype(np.float64) + np.nextafter(h, np.float16(s)).astype(np.float64)) / 2 for s in (-np.inf, np.inf)]
    return np.minimum(np.abs(X - mids[0]), np.abs(X - mids[1])) < PREDICATE_MARGIN


def f16_distance_bits(P, O):
    """The reference's distance pipeline (entity.py:206-210) on NumPy float16: the point and the origin are rounded to float16
    before they are subtracted, the difference and the hypotenuse are float16 operations."""
    p16, o16 = np.asarray(P, np.float64).astype(np.float16), np.asarray(O, np.float64).astype(np.float16)
    dx, dy = p16[:, 0] - o16[:, 0], p16[:, 1] - o16[:, 1]
    out = np.hypot(dx, dy)
    assert out.dtype == np.float16
    return out.view(np.uint16)


# ---- the truth of one configuration -----------------------------------------------------------------------------------------------
class Truth:
    def __init__(self, hulls, *, n_cops, n_thieves, n_rays, ray_length=400.0, ray_radius=1.0, agent_radius=5.0, wall_radius=1.0,
                 termination_radius=20.0, bbtree_gate=1, starts=None, regions=None):
        self.hulls = [np.asarray(h, np.float64) for h in hulls]
        self.S, self.nc, self.A, self.R = len(self.hulls), n_cops, n_cops + n_thieves, n_rays
        self.ray_length, self.ray_radius, self.agent_radius = float(ray_length), float(ray_radius), float(agent_radius)
        self.wall_radius, self.termination_radius, self.gated = float(wall_radius), float(termination_radius), bool(bbtree_gate)
        self.starts, self.regions = starts, regions
        ang = np.linspace(0.0, 2.0 * np.pi, n_rays, endpoint=False)      # entity.py:182-193: the fan covers the full circle
        self.dirs = np.stack([self.ray_length * np.cos(ang), self.ray_length * np.sin(ang)], 1)
        self.boxes = [np.concatenate([h.min(0) - self.wall_radius, h.max(0) + self.wall_radius]) for h in self.hulls]

    def observe(self, pos, tc, leaf_bb, ray_radius=None):
        """The expected outputs of every ray of every agent of every env, from the state at the START of the tick:
        ``hit_shape`` [N, A, R] (-1: none), ``obs_type``, ``obs_distance`` (float16 bits) and ``clear`` (see the module text)."""
        rr = self.ray_radius if ray_radius is None else float(ray_radius)
        pos, tc, leaf_bb = (np.asarray(x, np.float64) for x in (pos, tc, leaf_bb))
        N, A, R, S = pos.shape[0], self.A, self.R, self.S
        O = np.repeat(pos.reshape(N * A, 2), R, axis=0)
        D = np.tile(self.dirs, (N * A, 1))
        env = np.repeat(np.arange(N), A * R)
        me = np.tile(np.repeat(np.arange(A), R), N)
        M = len(O)
        alpha = np.full((M, S + A), np.inf)
        tbb = np.full((M, S + A), np.inf)
        marginal = np.zeros(M, bool)
        for s, V in enumerate(self.hulls):
            if self.gated:
                tbb[:, s], mg = gate(self.boxes[s], O, D)
                marginal |= mg
            else:
                tbb[:, s] = 0.0
            sel = np.flatnonzero(tbb[:, s] < 1.0)
            if len(sel):
                alpha[sel, s], mg = wall_alpha(V, self.wall_radius + rr, O[sel], D[sel])
                marginal[sel] |= mg
        for j in range(A):
            sel = np.flatnonzero(me != j)                                 # an agent's rays pass through its own disc
            if self.gated:
                t, mg = gate(leaf_bb[env[sel], j], O[sel], D[sel])
                marginal[sel] |= mg
            else:
                t = np.zeros(len(sel))
            tbb[sel, S + j] = t
            sel = sel[t < 1.0]
            if len(sel):
                alpha[sel, S + j], mg = disc_alpha(tc[env[sel], j], self.agent_radius + rr, O[sel], D[sel])   # the CACHED centre (Q1)
                marginal[sel] |= mg
        cand = np.where(tbb < 1.0, alpha, np.inf)
        rows = np.arange(M)
        w = np.argmin(cand, axis=1)
        a_w = cand[rows, w]
        hit = np.isfinite(a_w)
        rest = cand.copy()
        rest[rows, w] = np.inf
        clear = ~marginal & (~hit | (rest.min(axis=1) > np.maximum(a_w, tbb[rows, w]) + DELTA))
        shape = np.where(hit, w, -1)
        kind = np.where(~hit, EMPTY, np.where(w < S, WALL, np.where(w - S >= self.nc, THIEF, COP)))
        P = O + D                                                          # alpha 0: the segment's END is the point
        bits = np.full(M, np.array([self.ray_length]).astype(np.float16).view(np.uint16)[0], np.uint16)
        moving = hit & (a_w > 0.0)
        Cm = O + np.where(moving, a_w, 0.0)[:, None] * D
        near = Cm.copy()
        for s in np.unique(w[moving]):
            sel = np.flatnonzero(moving & (w == s))
            near[sel] = hull_distance(self.hulls[s], Cm[sel])[1] if s < S else tc[env[sel], s - S]
        away = Cm - near
        with np.errstate(divide="ignore", invalid="ignore"):
            unit = away / np.hypot(away[:, 0], away[:, 1])[:, None]
        P = np.where(moving[:, None], Cm - rr * unit, P)
        bits[hit] = f16_distance_bits(P[hit], O[hit])
        clear &= ~(hit & f16_tie(P).any(axis=1))
        sh = (N, A, R)
        return dict(hit_shape=shape.reshape(sh).astype(np.int32), obs_type=kind.reshape(sh).astype(np.uint8),
                    obs_distance=bits.reshape(sh), clear=clear.reshape(sh))

    def capture(self, pos):
        """-> (captured [N], marginal [N]): a cop and a thief closer than the termination radius (strictly, fresh positions) whose
        thin connecting segment stays farther than the wall radius from every hull."""
        pos = np.asarray(pos, np.float64)
        N = pos.shape[0]
        pairs = [(c, t) for t in range(self.nc, self.A) for c in range(self.nc)]
        Pc = np.concatenate([pos[:, c] for c, _ in pairs])
        Pt = np.concatenate([pos[:, t] for _, t in pairs])
        gap = np.hypot(*(Pc - Pt).T)
        wall = np.full(len(gap), np.inf)
        for V in self.hulls:
            wall = np.minimum(wall, segment_hull_distance(V, Pt, Pc))
        # (the nearest wall decides; another wall within the margin of the threshold would be nearer than that or blocked already)
        near, seen = gap < self.termination_radius, wall > self.wall_radius
        unsure = (np.abs(gap - self.termination_radius) < PREDICATE_MARGIN) | (np.abs(wall - self.wall_radius) < PREDICATE_MARGIN)
        fold = lambda x: x.reshape(len(pairs), N).any(axis=0)
        return fold(near & seen), fold(unsure)

    def spawn_ok(self, p, agent, tc_env):
        """Is ``p`` a position the spawn rule can give ``agent`` while the other agents' cached centres are ``tc_env`` [A, 2]?
        Without regions: the start position.  Else, inside one of the regions and either that region's centre (the fallback after
        the rejected draws) or free: every wall's surface and every other agent's disc at least one agent radius away."""
        p = np.asarray(p, np.float64)
        regs = self.regions[agent]
        if not regs:
            return bool(np.array_equal(p, self.starts[agent]))
        inside = [(x, y, w, h) for x, y, w, h in regs if x <= p[0] <= x + w and y <= p[1] <= y + h]
        if not inside:
            return False
        if any(p[0] == x + w / 2 and p[1] == y + h / 2 for x, y, w, h in inside):
            return True
        eps = PREDICATE_MARGIN                                            # two float64 evaluations of one distance differ by ~1e-13
        walls = all(hull_distance(V, p)[0] - self.wall_radius >= self.agent_radius - eps for V in self.hulls)
        others = all(np.hypot(*(p - tc_env[j])) - self.agent_radius >= self.agent_radius - eps for j in range(self.A) if j != agent)
        return walls and others
