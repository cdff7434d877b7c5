"""Cases for the pooled kernels' front and ray round (tests/test_pool_round_flat_host.py, tests/test_gpu_pool_round_flat.py).

Each case is there for a situation of `pool_sort` / `pool_round`, and asserts from the oracle's own run that the situation occurs in it:

    labyrinth_2v1_r64             the headline shape: one group of three chunks per front, rays with one and with several candidates
    labyrinth_inside_2v1_r64      every agent spawned inside the maze: nearly every ray has a candidate (the fullest ring), lists of four
    labyrinth_dense_2v1_r64       agents put where their rays meet most walls: the most live candidates per round that the map gives
    grandbyrinth_3v2_r64          five chunks (two groups of chunks in a front), four dynamic candidates per ray at most
    labyrinth_2v1_r90_exact_ring  six chunks, the ring of exact capacity
    squarinth_1v1_r90             one agent pair at 90 rays
    labyrinth_2v1_r64_generic     the generic (DynDims) kernels
    labyrinth_cones_2v1_r64       agents placed within each other's cones behind candidate walls: dynamic candidates at positions >= 1

What is counted (`Trace.situations`), per tick from the oracle's state at the tick's start: the ray's candidate walls from the library's own table
(cat_grid_lookup_host at the cell size the plan chose: the row the kernel reads), the walls among them whose bb the ray enters (t_bb < 1: live at a
pass's start), the other agents whose leaf bb it enters (inside the ray's cone: dynamic candidates, which stand behind the walls in a list).  A case is
run on the oracle once per process: spawn at injected positions, eight ticks of the oracle's random actions; the GPU tests replay that."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from as_cops_and_thieves_amd import _native as nat, tables
from as_cops_and_thieves_amd.config import C_FIELDS_F64, C_FIELDS_I32, SimConfig
from as_cops_and_thieves_amd.maps import load_preset
from oracle.cat_oracle import OracleSim
from tests import plan_cases as pc
from tests.util import free_positions

TICKS = 8
ROUND, MIN_PARTIAL, ITEM_CAP, PASS_J = 60, 40, 128, 8    # kPoolRound, kPoolMinPartial, kItemCap, kPassJ
OBS_KEYS = ("obs_distance", "obs_type", "hit_shape", "shared_distance", "shared_type", "team_positions")
# name -> map, cops, thieves, rays, envs, seed of the positions, how they are placed, knobs (environment of cat_create), situations that must occur
CASES = {
    "labyrinth_2v1_r64": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=40, seed=1, place="spread", env={}, need=("further",)),
    "labyrinth_inside_2v1_r64": dict(map="labyrinth-inside", cops=2, thieves=1, rays=64, n=40, seed=6, place="spawn", env={"CAT_POOL": "1"},
                                     need=("further", "second_flat_pass")),
    "labyrinth_dense_2v1_r64": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=20, seed=7, place="dense", env={"CAT_POOL": "1"}, need=("over_item_cap",)),
    "grandbyrinth_3v2_r64": dict(map="grandbyrinth", cops=3, thieves=2, rays=64, n=16, seed=3, place="spread", env={"CAT_POOL": "1"}, need=("past_pass_j",)),
    "labyrinth_2v1_r90_exact_ring": dict(map="labyrinth", cops=2, thieves=1, rays=90, n=20, seed=2, place="spread", env={}, need=("further",)),
    "squarinth_1v1_r90": dict(map="squarinth", cops=1, thieves=1, rays=90, n=20, seed=4, place="spread", env={"CAT_POOL": "1"}, need=("further",)),
    "labyrinth_2v1_r64_generic": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=20, seed=5, place="spread", env={"CAT_POOL": "1", "CAT_GENERIC_KERNEL": "1"},
                                      need=("further",)),
    "labyrinth_cones_2v1_r64": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=20, seed=8, place="cones", env={"CAT_POOL": "1"}, need=("dynamic_behind_wall",)),
}
MINIMUM = dict(wall=10000, agent=150, empty=1000)   # ray results over the whole trace, by kind: every case
DYNAMIC_BEHIND_WALL = 1000                         # rays (over the trace) with an agent in their cone behind at least one candidate wall of their list


def entered(a, d, boxes):
    """[R, S] bool: the segment a -> a + d[k] enters box s (l, b, r, t) with t_bb < 1"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tmin = np.full((len(d), len(boxes)), -np.inf)
        tmax = np.full_like(tmin, np.inf)
        ok = np.ones_like(tmin, bool)
        for ax in (0, 1):
            dd, lo, hi = d[:, ax][:, None], boxes[:, ax][None, :], boxes[:, ax + 2][None, :]
            t1, t2 = (lo - a[ax]) / dd, (hi - a[ax]) / dd
            par = dd == 0
            ok &= ~(par & ((a[ax] < lo) | (a[ax] > hi)))
            tmin = np.where(par, tmin, np.maximum(tmin, np.minimum(t1, t2)))
            tmax = np.where(par, tmax, np.minimum(tmax, np.maximum(t1, t2)))
    return ok & (tmin <= tmax) & (tmax >= 0) & (np.maximum(tmin, 0) < 1)


class Table:
    """the library's candidate table of one map, on the host (the rows the kernels read), at the plan's cell size"""

    def __init__(self, cfg, cmap, case):
        text = pc.describe_case(pc.PlanCase((case["map"],), case["cops"], case["thieves"], case["rays"], case["n"], env=case["env"]))
        kv = dict(ln.split("=", 1) for ln in text.splitlines())
        self.plan = kv
        c = nat.CatConfig()
        for n in C_FIELDS_I32 + C_FIELDS_F64:
            setattr(c, n, getattr(cfg, n))
        self.dx, self.dy = tables.ray_table(cfg.sensor)
        self.lut = np.zeros(32768, np.float32)
        t = nat.CatTables(self.dx.ctypes.data, self.dy.ctypes.data, self.lut.ctypes.data, self.lut.ctypes.data)
        blob = cmap.to_blob()
        self.h = C.c_void_p()
        assert nat.lib().cat_grid_build_host(C.byref(c), C.byref(t), blob, len(blob), 1.0 / float.fromhex(kv["part0.map0.inv_cell"]), C.byref(self.h)) == 0
        self.buf = (C.c_int * 256)()

    def row(self, x, y, k):
        n = nat.lib().cat_grid_lookup_host(self.h, float(x), float(y), k, self.buf, 256)
        return list(self.buf[:n])

    def close(self):
        nat.lib().cat_grid_free_host(self.h)


class Trace:
    def __init__(self, name):
        c = CASES[name]
        self.name, self.case = name, c
        self.cmap = load_preset(c["map"], c["cops"], c["thieves"]).compile()
        self.cfg = SimConfig(n_envs=c["n"], n_cops=c["cops"], n_thieves=c["thieves"], n_rays=c["rays"], max_step_count=10 ** 6, seed=17)
        cpu = OracleSim(self.cfg, [self.cmap])
        self.S = len(self.cmap.shape_bb)
        self.bb = np.asarray(self.cmap.shape_bb, np.float64)
        dx, dy = tables.ray_table(self.cfg.sensor)
        self.d = np.stack([dx, dy], 1)
        rng = np.random.default_rng(c["seed"])
        self.start = self._place(cpu, rng)
        self.reset_out = {k: np.array(v, copy=True) for k, v in cpu.reset(positions=self.start).items() if k in OBS_KEYS}
        self.state0 = {k: np.array(v, copy=True) for k, v in cpu.get_state().items()}
        self.actions = np.stack([cpu.random_actions(t) for t in range(TICKS)])
        self.outs, self.states = [], []
        for t in range(TICKS):
            out = cpu.step(self.actions[t])
            self.outs.append({k: np.array(v, copy=True) for k, v in out.items()})
            self.states.append({k: np.array(v, copy=True) for k, v in cpu.get_state().items()})

    # ---- placements
    def _place(self, cpu, rng):
        how, N, A = self.case["place"], cpu.N, cpu.A
        if how == "spawn":       # the preset's own spawn regions (labyrinth-inside: inside the maze)
            other = OracleSim(self.cfg, [self.cmap])   # (a sim of its own: the trace's sim is reset once, like the GPU's)
            other.reset()
            return other.get_state()["pos"].copy()
        pos = free_positions(cpu, self.cmap, rng, spread=60.0)
        if how == "dense":       # every agent at the best of 300 free points by walls entered per ray that enters any, 14 apart
            for e in range(N):
                cand = []
                for _ in range(300):
                    p = free_positions_one(cpu, self.cmap, rng, e)
                    g = entered(p, self.d, self.bb).sum(1)
                    cand.append((g.sum() / max((g > 0).sum(), 1), tuple(p)))
                cand.sort(reverse=True)
                chosen = []
                for _, p in cand:
                    if all(np.hypot(p[0] - q[0], p[1] - q[1]) >= 14.0 for q in chosen):
                        chosen.append(p)
                    if len(chosen) == A:
                        break
                pos[e] = np.array(chosen)
        if how == "cones":       # agent i + 1 beyond the first wall that a ray of agent i meets: in its cone, behind a candidate wall
            for e in range(N):
                for i in range(A - 1):
                    for _ in range(400):
                        k = int(rng.integers(len(self.d)))
                        u = self.d[k] / np.hypot(*self.d[k])
                        sh, alpha, _pt = cpu.segment_query(e, -2, pos[e, i], pos[e, i] + self.d[k], self.cfg.ray_radius)
                        if sh < 0 or sh >= self.S:
                            continue
                        q = pos[e, i] + (alpha * np.hypot(*self.d[k]) + rng.uniform(25.0, 60.0)) * u
                        if cpu.point_query_any(e, -2, q, 6.5) or any(np.hypot(*(q - pos[e, j])) < 13.0 for j in range(i + 1)):
                            continue
                        pos[e, i + 1] = q
                        break
        return pos

    # ---- what the inputs hold
    def counts(self):
        hs = np.stack([o["hit_shape"] for o in self.outs])
        return dict(wall=int(((hs >= 0) & (hs < self.S)).sum()), agent=int((hs >= self.S).sum()), empty=int((hs < 0).sum()))

    @functools.lru_cache(maxsize=None)
    def situations(self):
        """Over (tick, env): see the module's text.  Rates are per ACTIVE ray (a ray with a table row or a dynamic candidate: what enters the ring)."""
        tab = Table(self.cfg, self.cmap, self.case)
        A, R, N = self.start.shape[1], len(self.d), len(self.start)
        s = dict(further=0, longest_list=0, dynamic_behind_wall=0, best_further_per_round=0.0, best_live_per_min_partial=0.0)
        for t in range(TICKS):
            st = self.state0 if t == 0 else self.states[t - 1]
            for e in range(N):
                act = fur = live = 0
                for i in range(A):
                    a = st["pos"][e, i]
                    others = [j for j in range(A) if j != i]
                    walls_in = entered(a, self.d, self.bb)                                   # [R, S]
                    dyn_in = entered(a, self.d, st["leaf_bb"][e, others]).sum(1)             # [R]
                    for k in range(R):
                        row = tab.row(a[0], a[1], k)
                        n = len(row) + int(dyn_in[k])
                        if n == 0:
                            continue
                        act += 1
                        fur += n - 1
                        live += min(int(walls_in[k, row].sum()) + int(dyn_in[k]), PASS_J)
                        s["further"] += n > 1
                        s["longest_list"] = max(s["longest_list"], n)
                        s["dynamic_behind_wall"] += int(dyn_in[k] >= 1 and len(row) >= 1)   # a dynamic candidate at a position >= 1 of the list
                if act >= ROUND:
                    s["best_further_per_round"] = max(s["best_further_per_round"], fur * ROUND / act)
                    s["best_live_per_min_partial"] = max(s["best_live_per_min_partial"], live * MIN_PARTIAL / act)
        tab.close()
        return s

    def check(self):
        c = self.counts()
        for k, n in MINIMUM.items():
            assert c[k] >= n, (self.name, k, c)
        s = self.situations()
        for need in self.case["need"]:
            if need == "further":                  # rays with a candidate behind their first one
                assert s["further"] >= 1000, (self.name, s)
            # The three situations below were asked for as "more than 64 further pairs in a round", "more than 128 live items" and "lists past 8 positions".
            # With the tables the plan builds today no preset map reaches them (measured here, over every case: at most 26 further pairs per 60 rays of a
            # slot, 56 live candidates per 40, lists of 4), so each case asserts the most its map gives and the round's other paths (the position-major
            # loop for more than 64 pairs or a full item list, a second pass of kPassJ positions) stay covered by tests/test_gpu_parity.py's dense map only.
            elif need == "second_flat_pass":       # some slot tick: further pairs per 60 consecutive rays of the slot, on average
                assert s["best_further_per_round"] > 9.0 and s["longest_list"] >= 4, (self.name, s)
            elif need == "over_item_cap":          # some slot tick: live candidates per 40 consecutive rays of the slot, on average
                assert s["best_live_per_min_partial"] > 55.0, (self.name, s)
            elif need == "past_pass_j":            # the longest list, dynamic candidates included
                assert s["longest_list"] >= 4, (self.name, s)
            elif need == "dynamic_behind_wall":
                assert s["dynamic_behind_wall"] >= DYNAMIC_BEHIND_WALL, (self.name, s)
            else:
                raise KeyError(need)


def free_positions_one(cpu, cmap, rng, e, margin=6.5):
    W, H = cmap.window
    lo = np.maximum(cmap.shape_bb[:, :2].min(0) - 20, 8)
    hi = np.minimum(cmap.shape_bb[:, 2:].max(0) + 20, [W - 8, H - 8])
    for _ in range(10000):
        p = rng.uniform(lo, hi)
        if not cpu.point_query_any(e, -2, p, margin):
            return p
    raise RuntimeError("could not place agent")


@functools.lru_cache(maxsize=None)
def trace(name) -> Trace:
    return Trace(name)
