"""A scripted scenario that sits ON the two radius thresholds (tests/test_radius_thresholds_host.py, tests/test_gpu_radius_thresholds.py).

Labyrinth 2v1 at 64 rays (the pooled kernels), six envs, spawned at injected positions around one open point P; the cached circles and leaf
boxes the rays see (stale after a reset) are then set to the bodies' own places, and ONE tick runs:

    envs 0 1 2   the thief stands where its squared distance to cop 0 is the last double inside the capture radius, the first one
                 outside (sqrt(x) == termination_radius: not captured, the test is strict) and the next one
    envs 3 4 5   cop 1 stands where its squared distance to cop 0 is the last double with sqrt(x) - agent_radius <= ray_radius (the ray
                 origin counts as inside the other agent's circle: every ray towards it hits at alpha 0), the next one and the one after

The squared distances are hit EXACTLY: the offsets come from a search over neighbouring doubles of both coordinates, with the kernels' own
expression dx * dx + dy * dy.  The oracle (which takes the square root) says what each env must give; its flags and observations are checked
here, on the CPU, to really differ across each triple."""
from __future__ import annotations

import functools

import numpy as np

from as_cops_and_thieves_amd.config import SimConfig
from as_cops_and_thieves_amd.maps import load_preset
from oracle.cat_oracle import OracleSim

OBS_KEYS = ("obs_distance", "obs_type", "hit_shape", "shared_distance", "shared_type", "team_positions")
STILL = 0


def threshold_pair(term, rc, r2):
    """(X, E) by NumPy alone: bisection on the bit pattern with the old predicates (the library's values are compared with these on the host)"""
    def last_true(pred):
        lo, hi = 0, 0x7FF0000000000000
        if not pred(np.uint64(lo).view(np.float64)):
            return -1
        while lo < hi:
            mid = lo + (hi - lo + 1) // 2
            if pred(np.uint64(mid).view(np.float64)):
                lo = mid
            else:
                hi = mid - 1
        return lo
    inside = last_true(lambda x: np.sqrt(x) < term)
    near = last_true(lambda x: np.sqrt(x) - rc <= r2)
    return float(np.uint64(inside + 1).view(np.float64)), float(np.uint64(near).view(np.float64))


def offsets_for(p, radius, targets, span=400):
    """For each target squared distance: a point q near p + radius * (0.02, ~1) with fl(q - p) squared and summed == target exactly."""
    ang = 0.02
    q0 = p + radius * np.array([np.sin(ang), np.cos(ang)])
    steps = np.arange(-span, span + 1)
    xs = q0[0] + steps * np.spacing(q0[0])
    ys = q0[1] + steps * np.spacing(q0[1])
    dx, dy = (xs - p[0])[:, None], (ys - p[1])[None, :]
    d2 = dx * dx + dy * dy
    out = []
    for t in targets:
        hit = np.argwhere(d2 == t)
        assert len(hit), ("no neighbouring doubles give the squared distance", t, radius)
        i, j = hit[len(hit) // 2]
        out.append(np.array([xs[i], ys[j]]))
    return out


class Scenario:
    def __init__(self):
        self.cmap = load_preset("labyrinth", 2, 1).compile()
        self.cfg = cfg = SimConfig(n_envs=6, n_cops=2, n_thieves=1, n_rays=64, max_step_count=10 ** 6, seed=5)
        cpu = OracleSim(cfg, [self.cmap])
        self.X, self.E = threshold_pair(cfg.termination_radius, cfg.agent_radius, cfg.ray_radius)
        # an open point: no wall within 40 units, so every line of sight below is clear and no ray origin is near a wall
        rng = np.random.default_rng(3)
        W, H = self.cmap.window
        for _ in range(100000):
            P = np.floor(rng.uniform([60, 60], [W - 60, H - 60]))
            if not cpu.point_query_any(0, -2, P, 40.0):
                break
        else:
            raise RuntimeError("no open point on the map")
        self.P = P
        far = P + np.array([30.0, -25.0])       # out of every radius here, still in the open
        up = np.nextafter
        cap = offsets_for(P, cfg.termination_radius, [up(self.X, 0.0), self.X, up(self.X, np.inf)])
        nr = offsets_for(P, cfg.agent_radius + cfg.ray_radius, [self.E, up(self.E, np.inf), up(up(self.E, np.inf), np.inf)])
        start = np.zeros((6, 3, 2))
        for e in range(6):
            start[e, 0] = P
            if e < 3:
                start[e, 1], start[e, 2] = far, cap[e]
            else:
                start[e, 1], start[e, 2] = nr[e - 3], far
        self.start = start
        self.reset_out = {k: np.array(v, copy=True) for k, v in cpu.reset(positions=start).items() if k in OBS_KEYS}
        rc = cfg.agent_radius
        self.placed = dict(tc=start.copy(), leaf_bb=np.concatenate([start - rc, start + rc], -1))   # (l, b, r, t)
        cpu.set_state(**self.placed)
        self.actions = np.full((1, 6, 3), STILL, np.int32)
        out = cpu.step(self.actions[0])
        self.out = {k: np.array(v, copy=True) for k, v in out.items()}
        self.state = {k: np.array(v, copy=True) for k, v in cpu.get_state().items()}

    def d2(self, e, i, j):
        d = self.start[e, i] - self.start[e, j]
        return d[0] * d[0] + d[1] * d[1]

    def check(self):
        """the scenario is what it says: exact squared distances, and the oracle's results change exactly at the thresholds"""
        up = np.nextafter
        assert [self.d2(e, 2, 0) for e in range(3)] == [up(self.X, 0.0), self.X, up(self.X, np.inf)]
        assert [self.d2(e, 0, 1) for e in range(3, 6)] == [self.E, up(self.E, np.inf), up(up(self.E, np.inf), np.inf)]
        assert self.out["terminated"].astype(bool).tolist() == [True] + [False] * 5
        # near: every ray of cop 0 towards cop 1 hits at alpha 0, and the other way round -- the observations of env 3 differ from those of envs 4
        # and 5, which agree
        for i in (0, 1):
            a, b, c = (self.out["obs_distance"][3 + q, i] for q in range(3))
            assert not np.array_equal(a, b) and np.array_equal(b, c), i


@functools.lru_cache(maxsize=None)
def scenario() -> Scenario:
    return Scenario()
