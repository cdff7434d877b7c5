"""The scripted tapes on which a simulator (the CPU oracle, or the HIP library behind tests/gpu_sim.py) is held against the
mechanical truth of tests/step_truth.py, tick by tick.  ``make_sim(cfg, cmaps)`` is the switch, as in tests/ray_truth_cases.py.

A tape is a map, start positions and an action tape (tests/space_step_cases.py: the scripted policy runs ON THE ORACLE, once per
process, on the CPU).  A simulator replays it one tick per call with ``get_state`` after every tick; every tick's (state before,
actions, state after) then goes through the truth in one vectorised pass.  The truth reads the replaying simulator's own states, so
nothing of the oracle's trace is compared here.

The four traces of tests/space_step_cases.py are reused as they are; the further tapes run the same scripted policy on
``random_12`` (the slanted, touching and overlapping polygons of tests/ray_truth_cases.py), on ``lbirinth`` (5 px walls) and on the
dense ``agh-map``, and a ``bounce`` tape puts bodies a fraction of a pixel off a wall, or off each other, where they play patterns
that lose a contact and find it again within ``persistence`` ticks (the stale start of tests/step_truth.py)."""
from __future__ import annotations

import functools
import tempfile
import time
from pathlib import Path

import numpy as np

from tests import ray_truth as rt
from tests import ray_truth_cases as rc
from tests import space_step_cases as ssc
from tests.ray_truth_cases import oracle_sim
from tests.step_truth import StepTruth

MAX_NOT_CLEAR = 0.01      # of a case's agent-ticks (a condition on the case, met by the oracle alone: the seeds are chosen for it)
TOL_POS = 1e-9            # px
TOL_VEL = 1e-9            # px/s: vel and vbias.  Rounding: a few hundred ulps of values up to 1e3, divided by dt = 1/60, is about 1e-11
REPORT = []               # one line per finished case (pytest -s shows them; profiles/step_truth.txt is made of them)

# The further tapes.  name -> as in space_step_cases.CASES, plus `least`: what the tape's inputs must contain, counted by the truth's own geometry
# (the seeds were chosen on the CPU until it holds; tests/test_step_truth_host.py asserts it and prints the counts).
MORE = {
    "random_12_2v1": dict(map="random_12", cops=2, thieves=1, rays=64, n=20, ticks=150, seed=3, pool=None,
                          least=dict(single=500, vertex=20, slanted_edge=20)),
    "lbirinth_2v1": dict(map="lbirinth", cops=2, thieves=1, rays=64, n=20, ticks=150, seed=1, pool=None, least=dict(single=500)),
    "agh-map_2v1": dict(map="agh-map", cops=2, thieves=1, rays=64, n=16, ticks=150, seed=1, pool=None, least=dict(single=500, over_two_walls=5)),
    # 5 env slots: fewer than a workgroup has waves (the partly filled workgroup of the forced forms)
    "bounce_labyrinth_2v1": dict(map="labyrinth", cops=2, thieves=1, rays=64, n=5, ticks=150, seed=1, pool=None, bounce=True,
                                 least=dict(single=500, wall_refound_nonzero=5, pair_refound_nonzero=5, single_refound_nonzero=5)),
}
LEAST = {
    "labyrinth_2v1_mixed": dict(single=500, vertex=20, pair_and_wall=3),
    "labyrinth_2v1_units": dict(single=500, vertex=20, pair_and_wall=3),
    "squarinth_1v1": dict(single=500, pair_and_wall=3),
    "grandbyrinth_3v2": dict(single=500, pair_and_wall=3),
    **{k: v["least"] for k, v in MORE.items()},
}
CASES = list(LEAST)
# over all cases together (every figure of the list is also asked of the one case built for it, above)
LEAST_TOTAL = dict(vertex=20, slanted_edge=20, wall_refound=5, pair_refound=5, over_two_walls=5, pair_and_wall=3)

class BounceTrace(ssc.Trace):
    """Contacts that are lost and found again within ``persistence`` ticks.  An action adds 10 px/s and a contact takes the approaching
    velocity away, so from rest ``towards, away, towards`` repeated is: in (a sixth of a pixel; contact, at rest again), out, wait, in ...
    -- the entry is found again at age 2 with the impulse of the last contact still in it.  A body starts a fraction of that sixth
    off a wall and plays the pattern along the axis that leads to it; in the odd envs bodies 0 and 1 start in the open instead, a
    fraction of two sixths apart, and play it towards each other."""
    PATTERN = (0, 1, 0)       # offsets into (towards, away)

    def _place(self, cpu, rng, pos):
        hulls = rt.map_hulls(self.cmap.spec)
        rc_, rw = self.cfg.agent_radius, self.cfg.wall_radius
        step = np.array([(-1.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, -1.0)])
        self.axis = np.zeros((cpu.N, cpu.A), np.int64)           # the action that leads towards the wall (or the other body)
        for e in range(cpu.N):
            done = []
            if e % 2 == 1:
                for d in rng.permutation(4):
                    q = pos[e, 0] + step[d] * (2.0 * rc_ + rng.uniform(0.03, 0.3))
                    if not cpu.point_query_any(e, -2, q, rc_ + 2.0):
                        pos[e, 1], self.axis[e, 0], self.axis[e, 1] = q, d, (d + 2) % 4
                        break
                else:
                    raise RuntimeError("no room beside body 0")
                done = [0, 1]
            for i in range(len(done), cpu.A):
                for d in rng.permutation(4):
                    q = ssc._onto_wall(cpu, e, pos[e, i], int(d), rc_)
                    gap = min(rt.hull_distance(h, q)[0] for h in hulls) - (rc_ + rw)
                    q = q + step[d] * (gap - rng.uniform(0.02, 0.14))          # (the shift is exact in front of a face)
                    if gap < 0.5 and all(np.hypot(*(q - pos[e, j])) > 4.0 * rc_ for j in done):   # (a wall was met, away from the others)
                        pos[e, i], self.axis[e, i] = q, d
                        break
                else:
                    raise RuntimeError("no wall in any direction")
                done.append(i)
        return pos

    def _action(self, rng, t, e, i, st, mode):
        return int((self.axis[e, i] + 2 * self.PATTERN[t % len(self.PATTERN)]) % 4)


@functools.lru_cache(maxsize=None)
def trace(name) -> ssc.Trace:
    if name in ssc.CASES:
        return ssc.trace(name)
    c = MORE[name]
    with tempfile.TemporaryDirectory() as tmp:                   # (a random map is written out as the JSON file it is loaded from)
        cmap = rc.compiled_case_map(rc.Case(c["map"], cops=c["cops"], thieves=c["thieves"]), Path(tmp))
    return (BounceTrace if c.get("bounce") else ssc.Trace)(name, case=c, cmap=cmap)


def truth_for(cmap, cfg, **other) -> StepTruth:
    """The truth of a map and a configuration from plain data: the gift-wrapped hulls (held against the product's vertex sets by
    ray_truth_cases.truth_for) and plain numbers.  ``other`` replaces some of them (the sensitivity test)."""
    kw = dict(dt=cfg.dt, mass=cfg.agent_mass, impulse=cfg.impulse, max_speed=cfg.max_speed, agent_radius=cfg.agent_radius,
              wall_radius=cfg.wall_radius, bias_coef=cfg.bias_coef, slop=cfg.slop)
    kw.update(other)
    return StepTruth(rc.truth_for(cmap, cfg).hulls, **kw)


# ---- replaying a tape ------------------------------------------------------------------------------------------------------------
def _snap(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def replay(make_sim, tr, entry="step", auto_reset=False, check_kernel=None):
    """The tape on a simulator, one tick per call -> the states [T + 1] (``get_state`` before tick 0 and after every tick).
    ``entry``: "step", or "fused" (``step_fused``; the oracle has no such entry: its step, then its masked reset when ``auto_reset``,
    leave what the library's one launch leaves)."""
    sim = make_sim(tr.cfg, [tr.cmap])
    if check_kernel is not None:
        check_kernel(sim)
    sim.reset(positions=tr.start)
    sim.set_state(pos=tr.placed)
    states = [_snap(sim.get_state())]
    for a in tr.actions:
        if entry == "step":
            sim.step(a)
        elif hasattr(sim, "step_fused"):
            sim.step_fused(a, auto_reset=auto_reset)
        else:
            out = sim.step(a)
            if auto_reset:
                sim.reset(mask=np.array(out["terminated"], copy=True))
        states.append(_snap(sim.get_state()))
    if hasattr(sim, "device_errors"):
        assert sim.device_errors() == 0
    if hasattr(sim, "close"):
        sim.close()
    return states


KEYS = ("pos", "vel", "vbias", "wall_shape", "wall_age", "wall_jn", "pair_age", "pair_jn")


def against_truth(truth: StepTruth, states, actions):
    """Every tick of a replay through the truth in one pass.  A slot's tick is left out when its ``reset_count`` changed in it (the
    respawn of ``auto_reset`` moved its bodies).  -> (the truth's result over the kept slot ticks [B, A], kept [T, N])."""
    T, N = len(actions), len(actions[0])
    kept = np.stack([states[t + 1]["reset_count"] == states[t]["reset_count"] for t in range(T)])
    flat = kept.reshape(-1)
    fold = lambda rows, k: np.stack([s[k] for s in rows]).reshape(T * N, *np.shape(rows[0][k])[1:])[flat]
    before = {k: fold(states[:-1], k) for k in KEYS}
    after = {k: fold(states[1:], k) for k in KEYS}
    res = truth.tick(before, np.asarray(actions).reshape(T * N, -1)[flat], after)
    res["where"] = np.argwhere(kept)                              # row of the result -> (tick, env)
    return res, kept


def _worst(x, mask):
    x = np.where(mask, x, np.nan)
    return 0.0 if np.all(np.isnan(x)) else float(np.nanmax(x))


def summarise(name, res, seconds) -> dict:
    """The figures of one replay: counts, the not-clear share, the worst residual of every statement, the multi-contact figure."""
    c, clear = res["counts"], res["clear"]
    s = dict(name=str(name), counts=c, share=c["not_clear"] / max(c["agent_ticks"], 1), seconds=seconds,
             missing=len(res["missing"]), extra=len(res["extra"]), negative_jn=res["negative_jn"],
             pos=_worst(res["r_pos"], clear), vel=_worst(res["r_vel"], clear), free_vbias=_worst(res["r_free_vbias"], res["free"]),
             single_vel=_worst(res["r_single_vel"], res["single"]), single_vbias=_worst(res["r_single_vbias"], res["single"]),
             approach=0.0 if np.all(np.isnan(res["approach"])) else float(np.nanmin(res["approach"])))
    s["line"] = (f"step-truth {s['name']}: agent-ticks {c['agent_ticks']} not clear {c['not_clear']} ({100 * s['share']:.2f} %) free {c['free']} "
                 f"single {c['single']} multi {c['multi']} | wall contacts {c['wall_contacts']} (vertex {c['vertex']}, slanted edge {c['slanted_edge']}, "
                 f"re-found {c['wall_refound']}, of them stale > 0 {c['wall_refound_nonzero']}, on a single-contact body {c['single_refound_nonzero']}) "
                 f"pair contacts {c['pair_contacts']} (re-found {c['pair_refound']}, stale > 0 {c['pair_refound_nonzero']}) "
                 f"over two walls {c['over_two_walls']} pair and wall {c['pair_and_wall']} | missing {s['missing']} extra {s['extra']} negative jn {s['negative_jn']} | "
                 f"worst pos {s['pos']:.1e} vel {s['vel']:.1e} free vbias {s['free_vbias']:.1e} single vel {s['single_vel']:.1e} single vbias {s['single_vbias']:.1e} | "
                 f"multi-contact approach left {s['approach']:.3g} px/s | seconds {seconds:.2f}")
    return s


def first_of(res, key, tol, mask):
    bad = np.argwhere(np.where(mask, res[key], 0.0) > tol)
    return [dict(tick_env=tuple(int(x) for x in res["where"][b]), agent=int(a), residual=float(res[key][b, a])) for b, a in bad[:5]]


def hold(name, res, seconds=0.0) -> dict:
    """Print the figures, then assert: zero contact-set differences, no negative accumulated impulse, every residual of a clear body
    within the tolerance, the not-clear share within the cap."""
    s = summarise(name, res, seconds)
    REPORT.append(s["line"])
    print(s["line"])
    where = lambda rows: [(tuple(int(x) for x in res["where"][r[0]]), *r[1:]) for r in rows[:5]]
    assert not res["missing"], f"{name}: {len(res['missing'])} contacts of the truth have no age-0 cache entry ((tick, env), agent, hull): {where(res['missing'])}"
    assert not res["extra"], f"{name}: {len(res['extra'])} age-0 cache entries are no contact of the truth ((tick, env), agent, hull): {where(res['extra'])}"
    assert res["negative_jn"] == 0, f"{name}: {res['negative_jn']} accumulated impulses are negative"
    for key, tol, mask in (("r_pos", TOL_POS, "clear"), ("r_vel", TOL_VEL, "clear"), ("r_free_vbias", TOL_VEL, "free"),
                           ("r_single_vel", TOL_VEL, "single"), ("r_single_vbias", TOL_VEL, "single")):
        bad = first_of(res, key, tol, res[mask])
        assert not bad, f"{name}: {key} above {tol:g} on clear bodies, first {bad}"
    assert s["share"] <= MAX_NOT_CLEAR, f"{name}: {100 * s['share']:.2f} % of the agent-ticks are not clear (cap {100 * MAX_NOT_CLEAR:.0f} %)"
    return s


def run_case(make_sim, name, entry="step", auto_reset=False, check_kernel=None, tag=""):
    tr = trace(name)
    truth = truth_for(tr.cmap, tr.cfg)
    t0 = time.perf_counter()
    states = replay(make_sim, tr, entry, auto_reset, check_kernel)
    res, kept = against_truth(truth, states, tr.actions)
    s = hold(f"{name}{' [' + tag + ']' if tag else ''}", res, time.perf_counter() - t0)
    s["kept"] = kept
    return s


def check_least(name, counts) -> None:
    for k, n in LEAST[name].items():
        assert counts[k] >= n, (name, k, counts)


# ---- the stale start on a body that leaves ------------------------------------------------------------------------------------------
def stale_leave_case(make_sim):
    """Injected: the wall bodies of the bounce tape 0.3 px deep in their wall, moving AWAY from it at 10 px/s, with a cache entry of
    that wall aged 1 or 2 that still holds an impulse (4: less than the body's momentum, 25: more); the action is along the wall.
    The entry is found again, no warm start is applied, and the solver may draw the stale impulse down: the body is held back by
    min(stale / m, its leaving speed) -- the one place where the convention shows on a single contact that separates."""
    tr = trace("bounce_labyrinth_2v1")
    truth = truth_for(tr.cmap, tr.cfg)
    sim = make_sim(tr.cfg, [tr.cmap])
    sim.reset(positions=tr.start)
    st = _snap(sim.get_state())
    step = np.array([(-1.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, -1.0)])
    pos, vel = tr.placed.copy(), np.zeros_like(tr.placed)
    shape, age, jn = st["wall_shape"].copy(), st["wall_age"].copy(), st["wall_jn"].copy()
    actions = np.zeros(pos.shape[:2], np.int32)
    bodies = [(e, i) for e in range(pos.shape[0]) for i in range(2 if e % 2 else 0, pos.shape[1])]
    for q, (e, i) in enumerate(bodies):
        d = [rt.hull_distance(h, pos[e, i])[0] for h in truth.hulls]
        s = int(np.argmin(d))
        pos[e, i] += step[tr.axis[e, i]] * (d[s] - (truth.rc + truth.rw) + 0.3)
        vel[e, i] = -10.0 * step[tr.axis[e, i]]
        shape[e, i, 0], age[e, i, 0], jn[e, i, 0] = s, 1 + q % 2, (4.0, 25.0)[(q // 2) % 2]
        actions[e, i] = (tr.axis[e, i] + 1 + 2 * (q % 2)) % 4
    sim.set_state(pos=pos, vel=vel, wall_shape=shape, wall_age=age, wall_jn=jn)
    before = _snap(sim.get_state())
    sim.step(actions)
    after = _snap(sim.get_state())
    if hasattr(sim, "device_errors"):
        assert sim.device_errors() == 0
    if hasattr(sim, "close"):
        sim.close()
    res, _ = against_truth(truth, [before, after], actions[None])
    s = hold("a body leaving a re-found wall", res)
    assert s["counts"]["single_refound_nonzero"] == len(bodies) >= 8, s["counts"]
    v_in = truth.velocity_in(before["vel"], actions)
    held = np.array([np.hypot(*(after["vel"][e, i] - v_in[e, i])) for e, i in bodies])
    # (the check is not empty: every body is held back, some by the whole stale impulse 4 / m, some by all of their 10 px/s)
    assert held.min() > 1.0 and (np.abs(held - 4.0) < TOL_VEL).sum() >= 3 and (np.abs(held - 10.0) < TOL_VEL).sum() >= 3, held
    return s
