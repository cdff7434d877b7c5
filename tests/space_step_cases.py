"""Scripted scenarios for the Space.step tests (tests/test_space_step_host.py, tests/test_gpu_space_step_batch.py).

A case is a map, a roster, start positions and an action tape.  The tape comes from a small scripted policy that is run ON THE ORACLE
(push into a wall, run into a corner, chase another agent, retreat, stand still), so the oracle's trace -- every tick's outputs and state --
is produced on the CPU together with the tape, once per process, and the GPU tests replay the tape against it.  `coverage` counts, from the
oracle's states alone, what the inputs exercise: wall contacts, two contacts on one body, contacts on two bodies of an env, pair contacts,
bodies with more contacts than the register solver's bound, a pair contact together with a wall contact on one of the pair's bodies, cache entries that expire, and contact-free slot ticks that share a workgroup
with a contact slot.
"""
from __future__ import annotations

import functools

import numpy as np

from as_cops_and_thieves_amd.config import SimConfig
from as_cops_and_thieves_amd.maps import load_preset
from oracle.cat_oracle import OracleSim
from tests.util import free_positions

WPB = 16            # env slots of a workgroup (kMaxWaves)
SOLVE_REG = 2       # kSolveReg: most wall contacts of one body the register solver takes

# Where the labyrinth's wall shapes 0, 21 and 22 overlap (x 596 - 603, y 251 - 289) a body touches all three: more wall contacts on one body than the
# register solver takes, so the step runs the list-order loop on a wall-only list.  (env, agent, x, y), one per workgroup; the two square maps, four
# walls round a square, have no such place: at most two walls meet in their corners.
THREE_WALLS = ((2, 0, 599.5, 265.0), (17, 0, 600.0, 276.0))

# name -> map, cops, thieves, rays, envs, ticks, seed of the script, CAT_POOL, bodies put where three walls overlap, least over_bound count.  The seeds
# were chosen on the CPU until MINIMUM holds (test_space_step_host.py asserts it and prints the counts).
CASES = {
    "labyrinth_2v1_mixed": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=20, ticks=150, seed=1, pool="1", three_walls=THREE_WALLS, over_bound=5),
    "labyrinth_2v1_units": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=20, ticks=150, seed=1, pool="0", three_walls=THREE_WALLS, over_bound=5),
    "squarinth_1v1": dict(map="squarinth", cops=1, thieves=1, rays=90, n=16, ticks=150, seed=2, pool=None),
    "grandbyrinth_3v2": dict(map="grandbyrinth", cops=3, thieves=2, rays=64, n=16, ticks=150, seed=6, pool=None),
}
# what every case's inputs must contain (slot ticks, counted by `coverage`)
MINIMUM = dict(wall=20, two_on_one=5, two_agents=5, pair=3, pair_and_wall=3, wall_expired=3, pair_expired=3)
MIN_FREE_BESIDE_CONTACT = 0.25   # share of all slot ticks: contact-free, in a workgroup that has a contact slot in the same tick

OBS_KEYS = ("obs_distance", "obs_type", "hit_shape", "shared_distance", "shared_type", "team_positions")
STILL = (0, 2, 2, 0)   # velocities -10, 0, +10, 0: no net displacement


def _towards(d):
    """the action that pushes along the larger component of d (0: -x, 1: +y, 2: +x, 3: -y)"""
    if abs(d[0]) >= abs(d[1]):
        return 2 if d[0] > 0 else 0
    return 1 if d[1] > 0 else 3


def _onto_wall(cpu, e, p, d, rc):
    """from the free point p along direction d to the first point whose circle touches a wall (penetration below half a unit)"""
    step = np.array([(-1.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, -1.0)][d]) * 0.4
    q = p.copy()
    for _ in range(2000):
        if cpu.point_query_any(e, -2, q, rc - 0.1):
            return q
        q = q + step
    return p


class Trace:
    """``case`` / ``cmap``: a case record and a compiled map of the caller's (tests/step_truth_cases.py: maps that are no preset, other scripts);
    by default the case of that name above on its preset.  A subclass may place the bodies (``_place``) and script them (``_action``) differently."""

    def __init__(self, name, case=None, cmap=None):
        c = CASES[name] if case is None else case
        self.name, self.case = name, c
        self.cmap = load_preset(c["map"], c["cops"], c["thieves"]).compile() if cmap is None else cmap
        self.cfg = SimConfig(n_envs=c["n"], n_cops=c["cops"], n_thieves=c["thieves"], n_rays=c["rays"], max_step_count=10 ** 6, seed=11)
        cpu = OracleSim(self.cfg, [self.cmap])
        N, A, T = cpu.N, cpu.A, c["ticks"]
        rng = np.random.default_rng(c["seed"])
        self.start = free_positions(cpu, self.cmap, rng, spread=30.0)
        self.reset_out = {k: np.array(v, copy=True) for k, v in cpu.reset(positions=self.start).items() if k in OBS_KEYS}
        # envs 1 and 3 of every five stand still for the whole run (contact-free slots beside contact slots); in the others, every third body starts ON a wall
        self.calm = np.array([e % 5 in (1, 3) for e in range(N)])
        self.placed = pos = self._place(cpu, rng, cpu.get_state()["pos"].copy())
        cpu.set_state(pos=pos)
        self.actions = np.zeros((T, N, A), np.int32)
        self.outs, self.states = [], []
        mode = np.zeros((N, A, 3), np.int64)   # kind, argument, ticks left
        for t in range(T):
            st = cpu.get_state() if t == 0 else self.states[-1]
            for e in range(N):
                for i in range(A):
                    self.actions[t, e, i] = self._action(rng, t, e, i, st, mode)
            out = cpu.step(self.actions[t])
            self.outs.append({k: np.array(v, copy=True) for k, v in out.items()})
            self.states.append({k: np.array(v, copy=True) for k, v in cpu.get_state().items()})
        self.coverage = coverage(self.states)
        self.min_over_bound = c.get("over_bound", 0)

    def _place(self, cpu, rng, pos):
        """in the envs that are not calm, every third body starts ON a wall; the case's bodies where three walls overlap"""
        for e in range(cpu.N):
            for i in range(cpu.A):
                if not self.calm[e] and (e + i) % 3 == 0:
                    pos[e, i] = _onto_wall(cpu, e, pos[e, i], int(rng.integers(4)), self.cfg.agent_radius)
        for e, i, x, y in self.case.get("three_walls", ()):
            pos[e, i] = (x, y)
        return pos

    def _action(self, rng, t, e, i, st, mode):
        if self.calm[e]:
            return STILL[t % 4]
        A = mode.shape[1]
        if mode[e, i, 2] <= 0:
            mode[e, i] = (rng.choice(4, p=(0.3, 0.25, 0.3, 0.15)), rng.integers(4), rng.integers(10, 35))
            if mode[e, i, 0] == 2:
                mode[e, i, 1] = (i + 1 + rng.integers(A - 1)) % A
        kind, arg = mode[e, i, 0], mode[e, i, 1]
        mode[e, i, 2] -= 1
        if kind == 0:      # push one way (into a wall, or away from the one behind)
            return arg
        if kind == 1:      # into a corner: two neighbouring directions in turn
            return (arg + t % 2) % 4
        if kind == 2:      # chase body `arg`
            return _towards(st["pos"][e, arg] - st["pos"][e, i])
        return STILL[t % 4]


@functools.lru_cache(maxsize=None)
def trace(name) -> Trace:
    return Trace(name)


def coverage(states) -> dict:
    """Counts over (tick, env) from the oracle's states: a cache entry with age 0 is a contact of that tick's Space.step."""
    c = dict(slot_ticks=0, wall=0, two_on_one=0, two_agents=0, pair=0, over_bound=0, pair_and_wall=0, wall_expired=0, pair_expired=0, free_beside_contact=0)
    prev = None
    for st in states:
        live = (st["wall_shape"] >= 0) & (st["wall_age"] == 0)       # [N, A, K]
        per_agent = live.sum(-1)                                      # [N, A]
        pairs = (st["pair_age"] == 0).reshape(len(live), -1).sum(-1)  # [N]
        contact = (per_agent.sum(-1) > 0) | (pairs > 0)
        N = len(contact)
        c["slot_ticks"] += N
        c["wall"] += int((per_agent.sum(-1) > 0).sum())
        c["two_on_one"] += int((per_agent >= 2).any(-1).sum())
        c["two_agents"] += int(((per_agent > 0).sum(-1) >= 2).sum())
        c["pair"] += int(pairs.sum())
        c["over_bound"] += int((per_agent > SOLVE_REG).any(-1).sum())
        A, pi = per_agent.shape[1], 0
        mixed = np.zeros(len(live), bool)          # a pair contact and a wall contact on one of the pair's bodies: the mixed list
        for i in range(A):                          # pair index order of physics_env: (0,1), (0,2), ..., (1,2), ...
            for j in range(i + 1, A):
                mixed |= (st["pair_age"].reshape(len(live), -1)[:, pi] == 0) & ((per_agent[:, i] > 0) | (per_agent[:, j] > 0))
                pi += 1
        c["pair_and_wall"] += int(mixed.sum())
        for g in range(0, N, WPB):
            if contact[g:g + WPB].any():
                c["free_beside_contact"] += int((~contact[g:g + WPB]).sum())
        if prev is not None:
            c["wall_expired"] += int(((prev["wall_shape"] >= 0) & (st["wall_shape"] < 0)).sum())
            c["pair_expired"] += int(((prev["pair_age"] >= 0) & (st["pair_age"] < 0)).sum())
        prev = st
    return c


def check_coverage(c: dict, min_over_bound: int = 0) -> None:
    for k, n in MINIMUM.items():
        assert c[k] >= n, (k, c)
    assert c["over_bound"] >= min_over_bound, c
    assert c["free_beside_contact"] >= MIN_FREE_BESIDE_CONTACT * c["slot_ticks"], c
