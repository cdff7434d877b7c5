"""A mechanical ground truth for one tick of ``Space.step``, in NumPy float64: what the exposed state before a tick, the actions
and the exposed state after it must satisfy, whatever the solver did in between.

Written from mechanics and geometry, not from Chipmunk's functions and not from the kernels.  Nothing here restates a collision
routine or a Gauss-Seidel loop: the contact set comes from the DISTANCE FUNCTION of tests/ray_truth.py (a wall is the set of
points within ``wall_radius`` of a convex hull, an agent a disc), the normals from the closest points, and the impulses from the
accumulated values the state exposes.  For every (env, agent) of a tick, with m the mass and J the impulse of the action:

1. velocity in   ``v_in = clamp(vel_prev + J / m, max_speed)``.
2. position      ``pos = pos_prev + (v_in + vbias_prev) dt``.
3. contact set   wall s touches agent i iff ``hull_distance(hull_s, pos_i) < agent_radius + wall_radius``; a pair touches iff
                 ``|p_j - p_i| < 2 agent_radius``.  The cache entries with age 0 after the tick are exactly this set.
4. velocity out  ``vel = v_in + sum_k (dj_k / m) n_k``: n_k the geometric normal (a wall: (centre - closest hull point) /
                 distance; a pair: the centre line, equal and opposite on the two bodies), dj_k the impulse of this tick from the
                 accumulated ``jn`` of the state (below).  Every accumulated ``jn`` is >= 0.  Without a contact the sum is empty:
                 ``vel = v_in`` (statement 1 as observed) and ``vbias = 0``.
5. one contact   (one wall, no pair)  ``vel = v_in - min(s, v_in . n) n`` with s = 0 unless the entry started stale (below);
                 ``vbias = b n`` with ``b = -bias_coef min(0, gap + slop) / dt``, ``gap = distance - (agent_radius + wall_radius)``.

This module imports nothing from ``oracle`` and nothing from the product: hulls arrive as vertex arrays, the configuration as
plain numbers, states as arrays.

The ONE engine convention modelled, because a mechanical argument cannot replace it -- the STALE START.  Chipmunk keeps a contact
that was not found for up to ``persistence`` ticks.  When it is found again after ``age > 0`` its accumulated impulse starts from
the stale value, but no warm start is applied for it.  So, from the previous state's ages:
  a new entry                         starts at 0,         dj = jn_after;
  an entry with age 0 before the tick is warm-started,     dj = jn_after (its old impulse is applied again, then corrected);
  an entry with age > 0 before it     starts at jn_before, dj = jn_after - jn_before.
In statement 5 the same convention shows as s = jn_before / m for an entry of the third kind: the accumulator may be drawn down to
zero, so a body that LEAVES a re-found wall is held back by up to the stale impulse (s = 0 in the two other kinds, where the
statement is the plain inelastic contact: the tangent kept, the normal part zeroed only if approaching).

Not clear -- counted, not compared: an agent-tick with a gap, or a pair distance, within ``MARGIN`` of its threshold; a centre
inside a hull, at distance 0 (the product's documented deviation D4: no geometric normal exists there); the two bodies of a
coincident pair; and both bodies of a touching pair of which either is not clear for one of these reasons.
"""
from __future__ import annotations

import numpy as np

from tests.ray_truth import hull_distance

MARGIN = 1e-6            # the clear rule: gaps and pair distances against their thresholds (px)
ON_VERTEX = 1e-9         # a closest point this near a hull vertex lies ON it (coverage counting only)
# the action table of the reference's agents: 0: -x, 1: +y, 2: +x, 3: -y
ACTION_DIRS = np.array([(-1.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, -1.0)])


def pair_indices(A):
    """The pairs (i, j), i < j, in the order of the state's pair arrays: (0, 1), (0, 2), ..., (1, 2), ..."""
    return [(i, j) for i in range(A) for j in range(i + 1, A)]


def _feature(V, C):
    """Where on the hull ``V`` the closest points ``C`` [m, 2] lie -> (on a vertex [m], on an edge that is not axis-aligned [m])."""
    A, B = V, np.roll(V, -1, axis=0)
    on_vertex = np.hypot(C[:, None, 0] - A[None, :, 0], C[:, None, 1] - A[None, :, 1]).min(axis=1) < ON_VERTEX
    E = B - A
    t = np.clip(np.einsum("mkc,kc->mk", C[:, None, :] - A[None], E) / np.einsum("kc,kc->k", E, E), 0.0, 1.0)
    F = A[None] + t[..., None] * E[None]
    k = np.argmin(np.hypot(C[:, None, 0] - F[..., 0], C[:, None, 1] - F[..., 1]), axis=1)
    slanted = (np.abs(E[k, 0]) > ON_VERTEX) & (np.abs(E[k, 1]) > ON_VERTEX)
    return on_vertex, slanted & ~on_vertex


class StepTruth:
    def __init__(self, hulls, *, dt, mass, impulse, max_speed, agent_radius, wall_radius, bias_coef, slop):
        self.hulls = [np.asarray(h, np.float64) for h in hulls]
        self.S = len(self.hulls)
        self.dt, self.mass, self.impulse, self.max_speed = float(dt), float(mass), float(impulse), float(max_speed)
        self.rc, self.rw, self.bias_coef, self.slop = float(agent_radius), float(wall_radius), float(bias_coef), float(slop)

    # ---- statements 1 and 2 ------------------------------------------------------------------------------------------------------
    def velocity_in(self, vel_prev, actions):
        a = np.asarray(actions)
        J = np.where(((a >= 0) & (a <= 3))[..., None], ACTION_DIRS[np.clip(a, 0, 3)], 0.0) * self.impulse
        v = np.asarray(vel_prev, np.float64) + J / self.mass
        speed = np.hypot(v[..., 0], v[..., 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(speed > self.max_speed, self.max_speed / speed, 1.0)
        return v * scale[..., None]

    # ---- statement 3: the contact set, from the distance function ------------------------------------------------------------------
    def wall_contacts(self, pos):
        """Every (body, hull) whose distance is below the threshold or within MARGIN of it.  ``pos`` [M, 2] ->
        dict of flat arrays: body, hull, dist, normal [., 2] (0 inside a hull), touching, marginal, inside, on_vertex, slanted."""
        P = np.asarray(pos, np.float64).reshape(-1, 2)
        reach = self.rc + self.rw
        rows = dict(body=[], hull=[], dist=[], near=[], on_vertex=[], slanted=[])
        for s, V in enumerate(self.hulls):
            # (a hull lies inside its bounding box, so a point farther than the reach from the box is farther from the hull)
            cand = np.flatnonzero(np.all((P >= V.min(0) - reach - 1.0) & (P <= V.max(0) + reach + 1.0), axis=1))
            if not len(cand):
                continue
            d, c = hull_distance(V, P[cand])
            sel = d < reach + MARGIN
            if not sel.any():
                continue
            on_vertex, slanted = _feature(V, c[sel])
            for k, v in zip(rows, (cand[sel], np.full(int(sel.sum()), s), d[sel], c[sel], on_vertex, slanted)):
                rows[k].append(v)
        empty = dict(body=np.zeros(0, np.int64), hull=np.zeros(0, np.int64), dist=np.zeros(0), near=np.zeros((0, 2)),
                     on_vertex=np.zeros(0, bool), slanted=np.zeros(0, bool))
        w = {k: (np.concatenate(v) if v else empty[k]) for k, v in rows.items()}
        w["inside"] = w["dist"] == 0.0
        w["marginal"] = np.abs(w["dist"] - reach) < MARGIN
        w["touching"] = w["dist"] < reach
        with np.errstate(divide="ignore", invalid="ignore"):
            n = (P[w["body"]] - w["near"]) / w["dist"][:, None]
        w["normal"] = np.where(w["inside"][:, None], 0.0, n)
        return w

    # ---- one tick of many envs -------------------------------------------------------------------------------------------------------
    def tick(self, before, actions, after):
        """``before`` / ``after``: the exposed state (pos, vel, vbias [B, A, 2]; wall_shape, wall_age, wall_jn [B, A, K]; pair_age,
        pair_jn [B, NP]) before and after one tick of B envs (any mix of envs and ticks), ``actions`` [B, A].
        -> dict: per-agent [B, A] residuals ``r_pos`` (2), ``r_vel`` (4; 1 on a contact-free body), ``r_free_vbias``, ``r_single_vel``,
        ``r_single_vbias`` (5; nan where the statement does not apply), ``approach`` (the most negative normal velocity the solver left
        on a multi-contact body; nan elsewhere), the masks ``clear``, ``free``, ``single``, ``multi``, the contact-set differences
        ``missing`` / ``extra`` (lists of (env-row, agent, hull) and (env-row, pair)), ``negative_jn`` and the coverage ``counts``."""
        f = lambda d, k: np.asarray(d[k], np.float64)
        pos0, vel0, vb0, pos1, vel1, vb1 = f(before, "pos"), f(before, "vel"), f(before, "vbias"), f(after, "pos"), f(after, "vel"), f(after, "vbias")
        B, A = pos1.shape[:2]
        M, K = B * A, np.asarray(after["wall_shape"]).shape[-1]
        pairs = pair_indices(A)
        m, dt, reach = self.mass, self.dt, self.rc + self.rw
        ws0, wa0, wj0 = (np.asarray(before[k]).reshape(M, K) for k in ("wall_shape", "wall_age", "wall_jn"))
        ws1, wa1, wj1 = (np.asarray(after[k]).reshape(M, K) for k in ("wall_shape", "wall_age", "wall_jn"))
        pa0, pj0, pa1, pj1 = (np.asarray(d[k]).reshape(B, len(pairs)) for d in (before, after) for k in ("pair_age", "pair_jn"))

        v_in = self.velocity_in(vel0, actions)                                                       # 1
        r_pos = np.abs(pos1 - (pos0 + (v_in + vb0) * dt)).max(axis=-1)                               # 2

        # 3: walls
        w = self.wall_contacts(pos1)
        unclear = np.zeros(M, bool)
        unclear[w["body"][w["marginal"] | w["inside"]]] = True
        unclear = unclear.reshape(B, A)
        # 3: pairs
        pd = np.zeros((B, len(pairs)))
        pn = np.zeros((B, len(pairs), 2))
        for q, (i, j) in enumerate(pairs):
            d = pos1[:, j] - pos1[:, i]
            pd[:, q] = np.hypot(d[:, 0], d[:, 1])
            with np.errstate(divide="ignore", invalid="ignore"):
                pn[:, q] = np.where(pd[:, q, None] > 0.0, d / pd[:, q, None], 0.0)
        p_touch, p_marg, p_same = pd < 2.0 * self.rc, np.abs(pd - 2.0 * self.rc) < MARGIN, pd == 0.0
        for q, (i, j) in enumerate(pairs):
            unclear[:, i] |= p_marg[:, q] | p_same[:, q]
            unclear[:, j] |= p_marg[:, q] | p_same[:, q]
        own = unclear.copy()                                     # (not clear by itself; a touching pair passes it on once, not along a chain)
        for q, (i, j) in enumerate(pairs):
            either = (p_touch[:, q] | p_marg[:, q]) & (own[:, i] | own[:, j])
            unclear[:, i] |= either
            unclear[:, j] |= either
        clear = ~unclear
        clear_f = clear.reshape(M)

        # the cached sets: entries with age 0 after the tick
        live = (ws1 >= 0) & (wa1 == 0)
        assert ws1.max(initial=-1) < self.S, "a cache entry names a wall shape the map does not have"
        cached = np.zeros((M, self.S), bool)
        r, k = np.nonzero(live)
        cached[r, ws1[r, k]] = True
        truth = np.zeros((M, self.S), bool)
        truth[w["body"][w["touching"]], w["hull"][w["touching"]]] = True
        row = lambda a: [tuple(int(x) for x in (*divmod(int(b), A), int(s))) for b, s in np.argwhere(a)]
        missing = row(truth & ~cached & clear_f[:, None])
        extra = row(cached & ~truth & clear_f[:, None])
        p_live = pa1 == 0
        p_clear = np.stack([clear[:, i] & clear[:, j] for i, j in pairs], axis=1) if pairs else np.zeros((B, 0), bool)
        missing += [(int(b), ("pair", int(q))) for b, q in np.argwhere(p_touch & ~p_live & p_clear)]
        extra += [(int(b), ("pair", int(q))) for b, q in np.argwhere(p_live & ~p_touch & p_clear)]
        negative_jn = int(((ws1 >= 0) & (wj1 < 0.0)).sum() + ((pa1 >= 0) & (pj1 < 0.0)).sum())

        # 4: the impulses of this tick, from the accumulated values and the previous ages (the stale start)
        cb, cs = w["body"], w["hull"]
        eq1, eq0 = ws1[cb] == cs[:, None], ws0[cb] == cs[:, None]
        k1, k0 = eq1.argmax(axis=1), eq0.argmax(axis=1)
        solved = w["touching"] & ~w["inside"] & eq1.any(axis=1) & (wa1[cb, k1] == 0)
        w_stale = eq0.any(axis=1) & (wa0[cb, k0] > 0)
        w_start = np.where(w_stale, wj0[cb, k0], 0.0)
        w_dj = wj1[cb, k1] - w_start
        dv = np.zeros((M, 2))
        np.add.at(dv, cb[solved], (w_dj[solved] / m)[:, None] * w["normal"][solved])
        dv = dv.reshape(B, A, 2)
        p_solved = p_touch & p_live & ~p_same
        p_stale = pa0 > 0
        p_dj = pj1 - np.where(p_stale, pj0, 0.0)
        for q, (i, j) in enumerate(pairs):
            push = np.where(p_solved[:, q, None], (p_dj[:, q] / m)[:, None] * pn[:, q], 0.0)
            dv[:, i] -= push
            dv[:, j] += push
        r_vel = np.abs(vel1 - (v_in + dv)).max(axis=-1)

        n_wall = np.bincount(cb[w["touching"]], minlength=M).reshape(B, A)
        n_pair = np.zeros((B, A), np.int64)
        for q, (i, j) in enumerate(pairs):
            n_pair[:, i] += p_touch[:, q]
            n_pair[:, j] += p_touch[:, q]
        free = clear & (n_wall == 0) & (n_pair == 0)
        single = clear & (n_wall == 1) & (n_pair == 0)
        multi = clear & (n_wall + n_pair >= 2)
        r_free_vbias = np.where(free, np.abs(vb1).max(axis=-1), np.nan)

        # 5: the one wall contact of a single-contact body
        r_single_vel, r_single_vbias = np.full(M, np.nan), np.full(M, np.nan)
        one = np.flatnonzero(w["touching"] & single.reshape(M)[cb])
        b1, n1 = cb[one], w["normal"][one]
        vi = v_in.reshape(M, 2)[b1]
        vn = np.einsum("mc,mc->m", vi, n1)
        want_v = vi - np.minimum(w_start[one] / m, vn)[:, None] * n1
        bias = -self.bias_coef * np.minimum(0.0, (w["dist"][one] - reach) + self.slop) / dt
        r_single_vel[b1] = np.abs(vel1.reshape(M, 2)[b1] - want_v).max(axis=-1)
        r_single_vbias[b1] = np.abs(vb1.reshape(M, 2)[b1] - bias[:, None] * n1).max(axis=-1)

        # what the solver left on multi-contact bodies: the most negative normal velocity over a body's contacts
        approach = np.full(M, np.inf)
        np.minimum.at(approach, cb[solved], np.einsum("mc,mc->m", vel1.reshape(M, 2)[cb[solved]], w["normal"][solved]))
        approach = approach.reshape(B, A)
        for q, (i, j) in enumerate(pairs):
            rel = np.where(p_solved[:, q], np.einsum("bc,bc->b", vel1[:, j] - vel1[:, i], pn[:, q]), np.inf)
            approach[:, i] = np.minimum(approach[:, i], rel)
            approach[:, j] = np.minimum(approach[:, j], rel)
        approach = np.where(multi & np.isfinite(approach), approach, np.nan)

        seen = w["touching"] & clear_f[cb]                       # coverage: counted from this module's own geometry, on clear bodies
        a_of = np.array([p[0] for p in pairs] or [0]), np.array([p[1] for p in pairs] or [0])
        p_ok = p_touch & p_clear
        with_wall = p_ok & ((n_wall[:, a_of[0]] > 0) | (n_wall[:, a_of[1]] > 0)) if pairs else p_ok
        counts = dict(agent_ticks=M, not_clear=int(unclear.sum()), free=int(free.sum()), single=int(single.sum()), multi=int(multi.sum()),
                      wall_contacts=int(seen.sum()), pair_contacts=int(p_ok.sum()),
                      vertex=int((seen & w["on_vertex"]).sum()), slanted_edge=int((seen & w["slanted"]).sum()),
                      wall_refound=int((seen & solved & w_stale).sum()), wall_refound_nonzero=int((seen & solved & w_stale & (w_start > 0.0)).sum()),
                      pair_refound=int((p_ok & p_solved & p_stale).sum()), pair_refound_nonzero=int((p_ok & p_solved & p_stale & (pj0 > 0.0)).sum()),
                      single_refound_nonzero=int((w_stale[one] & (w_start[one] > 0.0)).sum()),
                      over_two_walls=int((clear & (n_wall > 2)).sum()), pair_and_wall=int(with_wall.sum()))
        return dict(clear=clear, free=free, single=single, multi=multi, r_pos=r_pos, r_vel=r_vel, r_free_vbias=r_free_vbias,
                    r_single_vel=r_single_vel.reshape(B, A), r_single_vbias=r_single_vbias.reshape(B, A), approach=approach,
                    missing=missing, extra=extra, negative_jn=negative_jn, counts=counts, n_wall=n_wall, n_pair=n_pair)
