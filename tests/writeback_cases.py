"""Scripted scenarios for tests/test_gpu_writeback_early.py: short episodes whose ticks reach every branch of a slot's write-back.

A case is a map, a roster, start positions, staggered step counters and an action tape.  Agents are put in each other's line of sight at a spread of
distances (so the non-terminal rewards are taken at many different sighting distances), one thief in every fifth env inside
the capture distance of cop 0 (an episode that ends by capture at tick 0), and ``max_step_count`` is small with the step counters of the slots of a
workgroup out of phase (episodes that end by time-out at different ticks).  The oracle plays the tape once per process; per tick it keeps what the tick
leaves BEFORE the episode's reset (what a launch without auto_reset hands back) and AFTER it (with auto_reset), outputs and state.  `coverage` counts, from
the oracle's outputs alone, the reward table indices per role, "no sighting" rewards, captures and time-outs.
"""
from __future__ import annotations

import functools

import numpy as np

from as_cops_and_thieves_amd import tables
from as_cops_and_thieves_amd.config import SimConfig
from as_cops_and_thieves_amd.maps import load_preset
from oracle.cat_oracle import OracleSim

MAX_STEP = 7
TICKS = 10
T_RESIDENT = 8
K_REPEAT = 3
TYPE_COP, TYPE_THIEF = 1, 2          # ObjectType (include/cat_sim.h)
OBS_KEYS = ("obs_distance", "obs_type", "shared_distance", "shared_type", "team_positions")
FLAG_KEYS = ("reward", "terminated", "truncated", "winner")

# name -> map, cops, thieves, rays, envs, CAT_POOL.  labyrinth at 40 envs: three workgroups of 16 slots, the last one partly filled.
CASES = {
    "labyrinth_2v1_pooled": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=40, pool="1", seed=1),
    "labyrinth_2v1_units": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=40, pool="0", seed=1),
    "squarinth_1v1": dict(map="squarinth", cops=1, thieves=1, rays=90, n=20, pool=None, seed=2),
    "grandbyrinth_3v2": dict(map="grandbyrinth", cops=3, thieves=2, rays=64, n=16, pool=None, seed=3),
}
MIN_INDICES = 32       # distinct reward table indices per role


def _copy(d, keys=None):
    return {k: np.array(v, copy=True) for k, v in d.items() if keys is None or k in keys}


def _open_line(cpu, e, a, b):
    """no wall within a unit of the segment a -> b (sampled every two units)"""
    n = int(np.hypot(*(b - a)) / 2.0) + 2
    return not any(cpu.point_query_any(e, -2, a + (b - a) * s, 1.0) for s in np.linspace(0.0, 1.0, n))


def _place(cpu, cmap, rng, n_cops):
    """cop 0 anywhere free; every other agent in an open line from cop 0, at a distance drawn log-uniformly from 22 .. 390 (the thief of every fifth env: at
    15, inside the capture distance); an agent for which no such place is found in 300 draws goes anywhere free."""
    N, A = cpu.N, cpu.A
    W, H = cmap.window
    lo = np.maximum(cmap.shape_bb[:, :2].min(0) - 20, 8)
    hi = np.minimum(cmap.shape_bb[:, 2:].max(0) + 20, [W - 8, H - 8])
    pos = np.zeros((N, A, 2))
    free = lambda e, p, taken: (lo <= p).all() and (p <= hi).all() and not cpu.point_query_any(e, -2, p, 6.5) and all(np.hypot(*(p - q)) >= 13.0 for q in taken)
    for e in range(N):
        while True:
            p0 = rng.uniform(lo, hi)
            if free(e, p0, []):
                break
        pos[e, 0] = p0
        for i in range(1, A):
            forced = e % 5 == 0 and i == n_cops
            for attempt in range(100000):
                if attempt < 300:
                    r = 15.0 if forced else float(np.exp(rng.uniform(np.log(22.0), np.log(390.0))))
                    ang = rng.uniform(0.0, 2.0 * np.pi)
                    p = p0 + r * np.array([np.cos(ang), np.sin(ang)])
                    ok = free(e, p, pos[e, :i]) and _open_line(cpu, e, p0, p)
                else:
                    if forced:
                        raise RuntimeError("no place inside the capture distance")
                    p = rng.uniform(lo, hi)
                    ok = free(e, p, pos[e, :i])
                if ok:
                    pos[e, i] = p
                    break
    return pos


def sightings(out, n_cops):
    """per (env, agent): the reward table index of a tick's outputs -- the smallest distance (f16 bits) among the rays that show the wanted class -- or -1"""
    d, ty = out["obs_distance"].astype(np.int64), out["obs_type"]
    A = d.shape[1]
    want = np.where(np.arange(A) < n_cops, TYPE_THIEF, TYPE_COP)[None, :, None]
    return np.where(ty == want, d, 1 << 20).min(-1), (ty == want).any(-1)


class Trace:
    def __init__(self, name):
        c = CASES[name]
        self.name, self.case = name, c
        self.cmap = load_preset(c["map"], c["cops"], c["thieves"]).compile()
        self.cfg = SimConfig(n_envs=c["n"], n_cops=c["cops"], n_thieves=c["thieves"], n_rays=c["rays"], max_step_count=MAX_STEP, seed=23)
        cpu = OracleSim(self.cfg, [self.cmap])
        N, A = cpu.N, cpu.A
        rng = np.random.default_rng(c["seed"])
        self.start = _place(cpu, self.cmap, rng, c["cops"])
        self.step_count = (np.arange(N) % MAX_STEP).astype(np.int32)
        self.actions = rng.integers(0, 4, size=(TICKS, N, A), dtype=np.int32)
        self.held = rng.integers(0, 4, size=(TICKS, N, A), dtype=np.int32)     # cat_step_repeat: one row per decision
        self.reset_out = _copy(cpu.reset(positions=self.start), OBS_KEYS)
        cpu.set_state(step_count=self.step_count)
        self.state0 = cpu.get_state()
        # ---- the tape, tick by tick: before and after the reset of the episodes that end
        self.pre, self.pre_state, self.post, self.post_state = [], [], [], []
        cop_lut, thief_lut = tables.cop_reward_lut().view(np.uint32), tables.thief_reward_lut().view(np.uint32)
        cov = dict(cop_idx=set(), thief_idx=set(), no_sighting=0, captured=0, timeout=0, running=0)
        for t in range(TICKS):
            out = _copy(cpu.step(self.actions[t]))
            self.pre.append(out)
            self.pre_state.append(cpu.get_state())
            term = out["terminated"] != 0
            cov["captured"] += int((out["winner"] == 0).sum()); cov["timeout"] += int((out["truncated"] != 0).sum()); cov["running"] += int((~term).sum())
            idx, seen = sightings(out, c["cops"])
            rew = out["reward"].view(np.uint32)
            for e in np.nonzero(~term)[0]:
                for i in range(A):
                    if not seen[e, i]:
                        cov["no_sighting"] += 1
                        continue
                    lut, key = (cop_lut, "cop_idx") if i < c["cops"] else (thief_lut, "thief_idx")
                    assert rew[e, i] == lut[idx[e, i]], (t, e, i)      # the oracle's reward IS the table entry of that index
                    cov[key].add(int(idx[e, i]))
            cpu.reset(mask=out["terminated"].copy())
            post = _copy(cpu.out)
            for k in FLAG_KEYS:
                post[k] = out[k]
            self.post.append(post)
            self.post_state.append(cpu.get_state())
        self.coverage = cov
        # ---- cat_step_repeat, K_REPEAT held ticks per decision from the same start: a slot stops at the tick that ends its episode (after its reset)
        cpu.reset(positions=self.start)
        cpu.set_state(**self.state0)
        self.repeat = []
        for d in range(TICKS // K_REPEAT):
            rows, states = [], []
            for j in range(K_REPEAT):
                out = _copy(cpu.step(self.held[d]))
                cpu.reset(mask=out["terminated"].copy())
                row = _copy(cpu.out)
                for k in FLAG_KEYS:
                    row[k] = out[k]
                rows.append(row); states.append(cpu.get_state())
            term = np.stack([r["terminated"] for r in rows]) != 0
            ended = term.any(0)
            jstar = np.where(ended, term.argmax(0), K_REPEAT - 1)
            pick = lambda seq: np.stack(seq)[jstar, np.arange(N)]
            want = {k: pick([r[k] for r in rows]) for k in rows[0] if k != "reward"}
            acc = rows[0]["reward"].copy()                      # the f32 left fold over the played ticks, one add at a time
            for j in range(1, K_REPEAT):
                acc = np.where((jstar >= j)[:, None], (acc + rows[j]["reward"]).astype(np.float32), acc)
            want["reward"] = acc
            want["ticks"] = (jstar + 1).astype(np.int32)
            state = {k: pick([s[k] for s in states]) for k in states[0]}
            cpu.set_state(**state)
            self.repeat.append(dict(want=want, state=state, jstar=jstar, ended=ended, captured=pick([r["winner"] for r in rows]) == 0))


@functools.lru_cache(maxsize=None)
def trace(name) -> Trace:
    return Trace(name)


def check_coverage(tr: Trace) -> None:
    c = tr.coverage
    assert len(c["cop_idx"]) >= MIN_INDICES and len(c["thief_idx"]) >= MIN_INDICES, (len(c["cop_idx"]), len(c["thief_idx"]))
    assert c["no_sighting"] > 0 and c["captured"] > 0 and c["timeout"] > 0 and c["running"] > 0, c
    term = np.stack([o["terminated"] for o in tr.pre]) != 0                    # [TICKS, N]
    assert term[1:T_RESIDENT - 1].any(), "no episode ends inside the resident launch"
    first = term[:, :16]
    assert (first.any(1) & ~first.all(1)).any(), "no tick at which slots of one workgroup end and others go on"
    early = any((r["ended"] & (r["jstar"] < K_REPEAT - 1)).any() for r in tr.repeat)
    full = any((~r["ended"]).any() for r in tr.repeat)
    by_capture = any((r["ended"] & r["captured"]).any() for r in tr.repeat)
    by_timeout = any((r["ended"] & ~r["captured"]).any() for r in tr.repeat)
    assert early and full and by_capture and by_timeout, (early, full, by_capture, by_timeout)
