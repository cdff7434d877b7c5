"""The scenarios in which a simulator (the CPU oracle, or the HIP library behind tests/gpu_sim.py) is held against the geometric
truth of tests/ray_truth.py.  ``make_sim(cfg, cmaps)`` is the switch, as in tests/test_oracle_known_answers.py.

Timing: a tick's observations, capture flag and winner belong to the state at the tick's START (the step observes before it
simulates), so every check reads ``get_state()``, then steps, then compares that step's outputs."""
from __future__ import annotations

import dataclasses
import time

import numpy as np

from as_cops_and_thieves_amd.config import SimConfig
from as_cops_and_thieves_amd.maps import Map, load_preset
from tests import ray_truth as rt
from tests.util import free_positions

MAX_EXCLUDED = 0.02       # of a case's rays (a condition on the case, met by the truth alone: the seeds are chosen for it)
OBS_KEYS = ("hit_shape", "obs_type", "obs_distance")
REPORT = []               # one line per finished case (pytest -s shows them; profiles/ray_truth.txt is made of them)


@dataclasses.dataclass
class Case:
    map: str
    rays: int = 64
    cops: int = 2
    thieves: int = 1
    envs: int = 8
    gate: int = 1
    ticks: int = 40             # K: random-action ticks before the checked tick
    max_steps: int = 30         # episode length: every slot times out (and respawns from the Philox stream) within K ticks
    seed: int = 1
    label: str = ""

    def __str__(self):
        return self.label or f"{self.map} {self.cops}v{self.thieves} R={self.rays} N={self.envs} gate={self.gate}"


# the five maps (rays and rosters as the flagship configurations run them); fewer envs on the dense map keep a case to seconds
FIVE_MAPS = [Case("labyrinth", envs=12), Case("lbirinth", envs=12),
             Case("squarinth", rays=90, cops=1, thieves=1, envs=12, ticks=60, max_steps=45),
             Case("grandbyrinth", cops=3, thieves=2, envs=8), Case("agh-map", envs=6)]
TREE_ORDER = [Case("lbirinth", envs=8, gate=2), Case("squarinth", envs=8, gate=2, ticks=60, max_steps=45)]
OTHERS = [Case("labyrinth", envs=4, gate=0, seed=6), Case("random_12", envs=8, seed=12),
          Case("labyrinth", rays=130, envs=8, seed=2)]
FEW_SLOTS = Case("labyrinth", envs=5, seed=2)          # fewer env slots than a workgroup has waves


def oracle_sim(cfg, cmaps):
    from oracle.cat_oracle import OracleSim
    return OracleSim(cfg, cmaps)


def compiled_case_map(case: Case, tmp_path=None):
    if case.map.startswith("random_"):
        import json
        from tests.test_spatial_grid import _random_polygon_map
        seed = int(case.map.split("_")[1])
        _random_polygon_map(tmp_path, seed, 14)
        f = tmp_path / f"random_{seed}.json"
        data = json.loads(f.read_text())
        for a in data["agents"]:
            a["spawn_region"] = {"x": 20, "y": 20, "w": 600, "h": 440}
        f.write_text(json.dumps(data))
        return Map(f).compile()
    return load_preset(case.map, case.cops, case.thieves).compile()


def config_for(case: Case, **kw) -> SimConfig:
    return SimConfig(n_envs=case.envs, n_cops=case.cops, n_thieves=case.thieves, n_rays=case.rays, max_step_count=case.max_steps,
                     seed=case.seed, bbtree_gate=case.gate, **kw)


def truth_for(cmap, cfg) -> rt.Truth:
    """The truth of a map and a configuration, from plain data.  Its gift-wrapped hulls must have the product's vertex sets."""
    hulls = rt.map_hulls(cmap.spec)
    assert len(hulls) == cmap.n_shapes
    for s, h in enumerate(hulls):
        theirs = cmap.planes[cmap.shape_first[s]:cmap.shape_first[s] + cmap.shape_count[s], 2:4]
        assert {tuple(v) for v in h.tolist()} == {tuple(v) for v in theirs.tolist()}, f"{cmap.name}: hull {s} differs"
    starts, regions = rt.agent_tables(cmap.spec)
    return rt.Truth(hulls, n_cops=cfg.n_cops, n_thieves=cfg.n_thieves, n_rays=cfg.n_rays, ray_length=cfg.ray_length,
                    ray_radius=cfg.ray_radius, agent_radius=cfg.agent_radius, wall_radius=cfg.wall_radius,
                    termination_radius=cfg.termination_radius, bbtree_gate=cfg.bbtree_gate, starts=starts, regions=regions)


class Tally:
    def __init__(self, name):
        self.name, self.rays, self.excluded, self.t0 = str(name), 0, 0, time.perf_counter()

    def rays_against_truth(self, truth, state, out, ctx, slots=None):
        """Every clear ray's hit shape, class and float16 distance bits equal the truth's: zero mismatches."""
        want = truth.observe(state["pos"], state["tc"], state["leaf_bb"])
        keep = want["clear"] if slots is None else want["clear"] & np.asarray(slots, bool)[:, None, None]
        n = want["clear"].size if slots is None else int(np.asarray(slots, bool).sum()) * want["clear"][0].size
        self.rays += n
        self.excluded += n - int(keep.sum())
        bad = keep & np.logical_or.reduce([np.asarray(out[k]) != want[k] for k in OBS_KEYS])
        if bad.any():
            where = np.argwhere(bad)
            first = [dict(at=tuple(int(i) for i in w), got=tuple(int(np.asarray(out[k])[tuple(w)]) for k in OBS_KEYS),
                          want=tuple(int(want[k][tuple(w)]) for k in OBS_KEYS)) for w in where[:5]]
            raise AssertionError(f"{self.name} [{ctx}]: {len(where)} clear rays differ from the geometric truth (env, agent, ray): {first}")

    def finish(self):
        share = self.excluded / max(self.rays, 1)
        line = f"ray-truth {self.name}: rays {self.rays} excluded {self.excluded} ({100 * share:.2f} %) mismatches 0 " \
               f"seconds {time.perf_counter() - self.t0:.2f}"
        REPORT.append(line)
        print(line)
        assert share <= MAX_EXCLUDED, f"{self.name}: {100 * share:.2f} % of the rays are not clear (cap {100 * MAX_EXCLUDED:.0f} %)"


def capture_against_truth(truth, state, out, ctx):
    """The captured flag (terminated and not timed out) and ``winner == 0`` equal the capture truth; no slot's decision is marginal."""
    captured, unsure = truth.capture(state["pos"])
    assert not unsure.any(), f"{ctx}: the capture decision of slots {np.flatnonzero(unsure).tolist()} is marginal"
    flag = (np.asarray(out["terminated"]) != 0) & (np.asarray(out["truncated"]) == 0)
    assert np.array_equal(flag, captured), f"{ctx}: captured flags {flag.astype(int).tolist()}, truth {captured.astype(int).tolist()}"
    assert np.array_equal(np.asarray(out["winner"]) == 0, captured), f"{ctx}: winner == 0 differs from the capture truth"
    return int(captured.sum())


def _snap(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def _close(sim):
    if hasattr(sim, "device_errors"):
        assert sim.device_errors() == 0
    if hasattr(sim, "close"):
        sim.close()


def _step_fused(sim, actions):
    """One tick with the finished slots respawned in the same call.  The oracle has no such entry: its step, then its masked reset,
    leave what the library's one launch leaves (tests/test_gpu_parity.py holds the two together)."""
    if hasattr(sim, "step_fused"):
        return _snap(sim.step_fused(actions, auto_reset=True))
    out = _snap(sim.step(actions))
    obs = sim.reset(mask=out["terminated"].copy())
    return {k: (np.array(obs[k], copy=True) if k in OBS_KEYS else v) for k, v in out.items()}


def _rollout_fused(sim, actions):
    if hasattr(sim, "rollout_fused"):
        return sim.rollout_fused(actions, auto_reset=True)
    rows = [_step_fused(sim, a) for a in actions]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def play(sim, truth, ticks, ctx, first_tick=0):
    """``ticks`` random-action ticks with the finished slots respawned; the capture truth is held at every one of them.
    -> (contacts seen, slots finished, captures)."""
    contacts = done = captures = 0
    for t in range(first_tick, first_tick + ticks):
        st = sim.get_state()
        out = sim.step(sim.random_actions(t))
        captures += capture_against_truth(truth, st, out, f"{ctx} tick {t}")
        ended = np.array(out["terminated"], copy=True)
        done += int(ended.sum())
        st = sim.get_state()
        contacts += int((st["wall_shape"] >= 0).sum() + (st["pair_age"] >= 0).sum())
        if ended.any():
            sim.reset(mask=ended)
    return contacts, done, captures


def reset_and_tick_case(make_sim, case: Case, tmp_path=None, check_kernel=None, tag=""):
    """Right after ``reset(positions=...)`` (agents near each other, caches stale) and at the tick that follows K random-action
    ticks in which contacts happened and slots ended and respawned."""
    cmap = compiled_case_map(case, tmp_path)
    cfg = config_for(case)
    sim, truth, tally = make_sim(cfg, [cmap]), truth_for(cmap, cfg), Tally(f"{case}{' [' + tag + ']' if tag else ''}")
    if check_kernel is not None:
        check_kernel(sim)
    pos = free_positions(oracle_sim(cfg, [cmap]), cmap, np.random.default_rng(case.seed), spread=60)
    out = _snap(sim.reset(positions=pos))
    tally.rays_against_truth(truth, sim.get_state(), out, "reset")
    contacts, done, _ = play(sim, truth, case.ticks, str(case))
    assert contacts > 0 and done > 0, f"{case}: {contacts} contacts, {done} finished slots in {case.ticks} ticks"
    st = sim.get_state()
    assert (st["reset_count"] >= 2).any()                                   # (a Philox respawn lies behind the checked state)
    out = _snap(sim.step(sim.random_actions(case.ticks)))
    tally.rays_against_truth(truth, st, out, f"tick {case.ticks}")
    capture_against_truth(truth, st, out, f"{case} tick {case.ticks}")
    _close(sim)
    tally.finish()
    return tally


def fused_step_case(make_sim, case: Case):
    """``step_fused(auto_reset=True)`` at a tick where some slots end and others do not.  A slot that ends leaves the NEW episode's
    observations: its rays start at the positions the launch leaves behind and meet the agents' discs where the tick's Space.step
    cached them (the respawn moves bodies, not caches), so the truth reads the state AFTER the launch for those slots, and the
    state before it for the others.  The flags belong to the tick's start for every slot."""
    cmap = compiled_case_map(case)
    cfg = config_for(case)
    sim, truth, tally = make_sim(cfg, [cmap]), truth_for(cmap, cfg), Tally(case)
    pos = free_positions(oracle_sim(cfg, [cmap]), cmap, np.random.default_rng(case.seed), spread=60)
    sim.reset(positions=pos)
    late = np.arange(case.envs) % 2 == 1                                    # the odd slots start their episode three ticks later
    for t in range(3):
        sim.step(sim.random_actions(t))
    sim.reset(mask=late.astype(np.uint8))
    for t in range(3, case.max_steps - 1):
        out = sim.step(sim.random_actions(t))
        sim.reset(mask=np.array(out["terminated"], copy=True))
    before = sim.get_state()
    out = _step_fused(sim, sim.random_actions(case.max_steps - 1))
    after = sim.get_state()
    ended = out["terminated"] != 0
    assert ended.any() and not ended.all(), ended.tolist()
    assert (out["truncated"][~late] != 0).any()                             # early slots reach the episode length at this tick
    capture_against_truth(truth, before, out, f"{case} fused tick")
    tally.rays_against_truth(truth, before, out, "slots that go on", slots=~ended)
    tally.rays_against_truth(truth, after, out, "slots that ended", slots=ended)
    _close(sim)
    tally.finish()
    return tally


def rollout_case(make_sim, case: Case, T=4):
    """``rollout_fused(T)``: row 0 against the state read before the launch (the later rows are tied to one-tick launches, bit for
    bit, by tests/test_gpu_rollout_resident.py)."""
    cmap = compiled_case_map(case)
    cfg = config_for(case)
    sim, truth, tally = make_sim(cfg, [cmap]), truth_for(cmap, cfg), Tally(case)
    pos = free_positions(oracle_sim(cfg, [cmap]), cmap, np.random.default_rng(case.seed), spread=60)
    sim.reset(positions=pos)
    play(sim, truth, case.ticks, str(case))
    before = sim.get_state()
    acts = np.stack([sim.random_actions(case.ticks + t) for t in range(T)])
    rows = _rollout_fused(sim, acts)
    row0 = {k: v[0] for k, v in rows.items()}
    assert not row0["terminated"].any(), "row 0 must end no slot (its observations would be the next episode's)"
    capture_against_truth(truth, before, row0, f"{case} rollout row 0")
    tally.rays_against_truth(truth, before, row0, "rollout row 0")
    _close(sim)
    tally.finish()
    return tally


# ---- capture by injection --------------------------------------------------------------------------------------------------------
def injected_pairs(truth: rt.Truth, starts, rng, per_class=4):
    """Positions [3 * per_class, A, 2] built from the hulls: cop 0 and the first thief (a) inside the termination radius across a
    wall -- straddling a thin wall where the map has one (thinner than the radius), else across the corner of a block --, (b) inside
    the radius in the open, (c) just outside the radius in the open.  Every other agent stands far away.  -> (positions, class)."""
    A, nc, R = truth.A, truth.nc, truth.termination_radius
    far = np.asarray(starts, np.float64)                                     # the others stay at their start positions, out of reach
    rows, kinds = [], []

    def row(pc, pt, kind):
        p = far.copy()
        p[0], p[nc] = pc, pt
        rows.append(p)
        kinds.append(kind)

    thin = [h for h in truth.hulls if min(np.ptp(h, axis=0)) + 2 * truth.wall_radius < R - 6.0]
    for q in range(per_class):
        if thin:                                                             # either side of the wall's thin axis, 3 px off its faces
            h = thin[q % len(thin)]
            axis = int(np.argmin(np.ptp(h, axis=0)))
            mid = (h.min(0) + h.max(0)) / 2
            mid[1 - axis] += (q - per_class / 2) * 7.0
            off = np.zeros(2)
            off[axis] = np.ptp(h, axis=0)[axis] / 2 + 3.0
            row(mid - off, mid + off, "blocked")
        else:                                                                # 8 px either way along the corner's tangent, 2 px into the block
            h = truth.hulls[(3 * q + 1) % truth.S]
            k = q % len(h)
            e0, e1 = h[k] - h[k - 1], h[(k + 1) % len(h)] - h[k]
            u = e0 / np.hypot(*e0) - e1 / np.hypot(*e1)                      # out of the corner, along its bisector
            u /= np.hypot(*u)
            tang = np.array([-u[1], u[0]])
            row(h[k] + 8.0 * tang - 2.0 * u, h[k] - 8.0 * tang - 2.0 * u, "blocked")
    lo = np.min([h.min(0) for h in truth.hulls], axis=0)
    hi = np.max([h.max(0) for h in truth.hulls], axis=0)
    for kind, gap in (("seen", 0.8 * R), ("outside", R + 0.5)):
        n = 0
        while n < per_class:
            p = rng.uniform(lo + 10, hi - 10)
            ang = rng.uniform(0, 2 * np.pi)
            q = p + gap * np.array([np.cos(ang), np.sin(ang)])
            if min(np.hypot(*(far - p).T).min(), np.hypot(*(far - q).T).min()) < 3 * R:
                continue
            if min(float(rt.segment_hull_distance(h, p, q)[0]) for h in truth.hulls) > truth.wall_radius + 2.0:
                row(p, q, kind)
                n += 1
    return np.array(rows), kinds


def capture_injection_case(make_sim, name, cops=2, thieves=1, seed=1):
    cmap = load_preset(name, cops, thieves).compile()
    probe = truth_for(cmap, SimConfig(n_cops=cops, n_thieves=thieves, n_rays=8))
    pos, kinds = injected_pairs(probe, probe.starts, np.random.default_rng(seed))
    cfg = SimConfig(n_envs=len(pos), n_cops=cops, n_thieves=thieves, n_rays=8, seed=seed)
    sim, truth = make_sim(cfg, [cmap]), truth_for(cmap, cfg)
    sim.reset(positions=pos)
    st = sim.get_state()
    assert np.array_equal(st["pos"], pos)
    out = _snap(sim.step(np.zeros((len(pos), cops + thieves), np.int32)))
    captured, unsure = truth.capture(pos)
    assert not unsure.any()
    for kind, want in (("blocked", False), ("seen", True), ("outside", False)):
        rows = [i for i, k in enumerate(kinds) if k == kind]
        assert len(rows) >= 3 and (captured[rows] == want).all(), (kind, captured[rows].tolist())
    gaps = np.hypot(*(pos[:, 0] - pos[:, cops]).T)
    assert all(g < cfg.termination_radius for g, k in zip(gaps, kinds) if k != "outside")
    capture_against_truth(truth, st, out, f"{name} injected pairs")
    _close(sim)
    line = f"capture-truth {name} {cops}v{thieves}: slots {len(pos)} ({', '.join(f'{k} {kinds.count(k)}' for k in ('blocked', 'seen', 'outside'))}) agree"
    REPORT.append(line)
    print(line)


# ---- spawn -----------------------------------------------------------------------------------------------------------------------
def spawn_case(make_sim, name, cops, thieves, envs=12, seed=3):
    """``reset()`` without positions, twice, with three ticks in between: the second respawn is tested against discs cached where the
    agents stood at the last Space.step, not where the first respawn put them."""
    cmap = load_preset(name, cops, thieves).compile()
    cfg = SimConfig(n_envs=envs, n_cops=cops, n_thieves=thieves, n_rays=8, seed=seed)
    sim, truth = make_sim(cfg, [cmap]), truth_for(cmap, cfg)
    checked = moved = 0
    for round_ in range(2):
        tc = sim.get_state()["tc"].copy()
        sim.reset()
        pos = sim.get_state()["pos"]
        for e in range(envs):
            for i in range(truth.A):
                assert truth.spawn_ok(pos[e, i], i, tc[e]), f"{name} reset {round_}: env {e} agent {i} at {pos[e, i].tolist()}"
                checked += 1
        moved += int((np.abs(pos - tc).max(axis=-1) > 0).sum())
        for t in range(3):
            sim.step(sim.random_actions(t))
    _close(sim)
    line = f"spawn-truth {name} {cops}v{thieves}: {checked} spawned positions agree ({moved} away from their cached discs)"
    REPORT.append(line)
    print(line)
    return checked, moved
