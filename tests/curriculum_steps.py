"""The GPU steps of tests/test_gpu_curriculum.py, one per process: ``python -m tests.curriculum_steps STEP`` (the helpers and the conventions
of tests/act_steps.py: a step prints its figures and exits 0 when every check holds, 1 with the failed checks listed).  The reference of
every comparison is ``navigation.spawn_step`` on the CPU, over a field whose hop table ``hops_reference`` built there."""
from __future__ import annotations

import sys

import numpy as np
import torch

from as_cops_and_thieves_amd import navigation as nv
from tests import curriculum_cases as cc
from tests.act_steps import FAILED, check, guarded

PATTERN = -12345.0625
t = torch.from_numpy


def intact(whole, band, fill):
    return bool((whole[:band] == fill).all()) and bool((whole[-band:] == fill).all())


# ---------------------------------------------------------------------------------------------- 1. the kernel on synthetic buffers
def synthetic_batch(rows, N, A, seed):
    mask, u, band, slot_map = cc.random_batch(seed, N, A)
    K = min(len(rows), N)
    if K:
        known = cc.batch(rows[:K], A)
        mask[:K], u[:, :K], band[:K], slot_map[:K] = known["mask"], known["uniform"], known["band"], known["slot_map"]
    return mask, u, band, slot_map, K


def step_synthetic():
    from as_cops_and_thieves_amd import _learn_native as ln
    placed_rows = fallback_rows = off_rows = 0
    for A, n_cops, rows in ((3, 2, cc.rows_2v1()), (3, 1, cc.rows_1v2()), (5, 3, [])):
        for N in (1, 63, 257):
            tag = f"A={A} n_cops={n_cops} N={N}"
            mask, u, band, slot_map, K = synthetic_batch(rows, N, A, 100 * A + 10 * n_cops + N)
            cpu, gpu = cc.make_field(slot_map), cc.make_field(slot_map, "cuda")
            check(all(np.array_equal(gpu.hops_of(m), cpu.hops_of(m)) for m in (0, 1)), f"{tag}: the two fields agree")
            want_pos, want_placed = torch.full((N, A, 2), PATTERN, dtype=torch.float64), torch.full((N,), 7, dtype=torch.uint8)
            nv.spawn_step(t(mask), t(u), t(band), cpu, n_cops, positions=want_pos, placed=want_placed)
            pos, pos_whole, guard = guarded((N, A, 2), torch.float64, PATTERN)
            placed, placed_whole, _ = guarded((N,), torch.uint8, 7)
            ln.nav_spawn(t(mask).cuda(), t(u).cuda(), t(band).cuda(), gpu, n_cops, pos, placed)
            torch.cuda.synchronize()
            check(torch.equal(placed.cpu(), want_placed), f"{tag}: placed bytes ({int((placed.cpu() != want_placed).sum())} differ)")
            check(torch.equal(pos.cpu().view(torch.int64), want_pos.view(torch.int64)), f"{tag}: f64 bits of positions "
                  f"({int((pos.cpu().view(torch.int64) != want_pos.view(torch.int64)).any(-1).any(-1).sum())} rows differ)")
            check(intact(pos_whole, guard, PATTERN) and intact(placed_whole, guard, 7), f"{tag}: guard bands intact")
            off = want_placed == 0
            check(bool((pos.cpu()[off] == PATTERN).all()), f"{tag}: unwritten rows keep their pre-fill")
            if K == len(rows) and K:                           # the hand-derived answers themselves, from the kernel
                known = cc.batch(rows, A)
                got = np.where((placed.cpu().numpy()[:K] == 1)[:, None, None], pos.cpu().numpy()[:K], np.nan)
                check(np.array_equal(placed.cpu().numpy()[:K], known["placed"]) and np.array_equal(got, known["positions"], equal_nan=True),
                      f"{tag}: the hand-derived rows")
            valid = (mask != 0) & (band[:, 0] >= 1) & (band[:, 0] <= band[:, 1]) & (band[:, 1] <= 65534)
            placed_rows += int(want_placed.sum()); fallback_rows += int((valid & off.numpy()).sum()); off_rows += int((~valid).sum())
    print(f"synthetic: {placed_rows} placed rows, {fallback_rows} fallbacks, {off_rows} rows off or unmasked", flush=True)
    check(placed_rows > 100 and fallback_rows > 50 and off_rows > 100, "placed rows, fallbacks and rows that do not take part all occur")
    # bad arguments are refused with real buffers, too
    gpu = cc.make_field(np.zeros(4, np.int32), "cuda")
    buf = lambda A: (torch.ones(4, dtype=torch.uint8, device="cuda"), torch.zeros(A, 4, device="cuda"), torch.full((4, 2), 2, dtype=torch.int32, device="cuda"))
    for A, n_cops, what in ((3, 0, "n_cops"), (3, 3, "n_cops"), (17, 2, "CAT_RENDER_MAX_AGENTS")):
        pos, placed = torch.full((4, A, 2), PATTERN, dtype=torch.float64, device="cuda"), torch.full((4,), 7, dtype=torch.uint8, device="cuda")
        try:
            ln.nav_spawn(*buf(A), gpu, n_cops, pos, placed)
            check(False, f"bad {what} is refused")
        except RuntimeError as exc:
            check(what in str(exc), f"bad {what} is refused with a message ({exc})")
        torch.cuda.synchronize()
        check(bool((pos == PATTERN).all()) and bool((placed == 7).all()), f"bad {what}: nothing was written")


# ---------------------------------------------------------------------------------------------- 2. against the env
def make_env(N=256, msc=8, seed=3, **kw):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    env = VecCopsEnv(load_preset("squarinth", 2, 1), N, num_rays=64, max_step_count=msc, seed=seed, final_positions=True, **kw)
    env.reset()
    return env


def fed_spawner(env, lo, hi):
    """A ``GeodesicSpawner`` whose ``respawn`` draws from ``feed`` (fp32 [A, N]) where no ``uniform`` is passed: the test decides the draws."""
    from as_cops_and_thieves_amd.selfplay.curriculum import GeodesicSpawner

    class Fed(GeodesicSpawner):
        feed = None

        def respawn(self, raw, uniform=None):
            return super().respawn(raw, self.feed if uniform is None else uniform)

    return Fed(env, lo, hi)


KEEP = ("reward", "terminated", "truncated", "winner", "final_positions")


def run_env_pair(repeat, ticks=24, N=256):
    """Env A carries the spawner; env B has none and is driven by hand (the same actions, then ``reset`` with the definition's outputs); env C
    has none either: ``step_fused`` / ``step_repeat``, a clone of the terminal tick's rows, then ``respawn`` by hand."""
    a, b, c = make_env(N), make_env(N), make_env(N)
    sa, sc_ = fed_spawner(a, 2, 6), fed_spawner(c, 2, 6)
    a.set_spawner(sa)
    cpu = nv.NavField.from_maps(a._compiled, a.slot_map_ids, 16, 6.0, "cpu", arena=True)
    check(np.array_equal(cpu.hops_of(0), sa.field.hops_of(0)) and np.array_equal(cpu.free_of(0), sa.field.free_of(0)), "the CPU field equals the spawner's")
    band = torch.full((N, 2), 2, dtype=torch.int32); band[:, 1] = 6
    gen = torch.Generator().manual_seed(9)
    kw = {} if repeat == 1 else {"repeat": repeat}
    terminal = bad_out = bad_state = bad_keep = bad_placed = 0
    for tick in range(ticks):
        actions = torch.randint(0, 4, (N, 3), generator=gen, dtype=torch.int32).cuda()
        u = torch.rand(3, N, generator=gen)
        sa.feed = sc_.feed = u.cuda()
        ra = a.step_raw(actions, **kw)
        rb = b.step_raw(actions, **kw)
        term = rb["terminated"].cpu()
        pos, placed = nv.spawn_step(term, u, band, cpu, 2)
        b.reset(options={"mask": placed.cuda(), "positions": pos.cuda()})
        rc = c._sim.step_fused(actions) if repeat == 1 else c._sim.step_repeat(actions, repeat)
        clone = {k: rc[k].clone() for k in KEEP}
        sc_.respawn(rc)
        torch.cuda.synchronize()
        n_term = int((term != 0).sum())
        terminal += n_term
        bad_placed += int(int(placed.sum()) != n_term or not torch.equal(sa.placed.cpu(), placed))
        outs_b, outs_c = b.raw_outputs(), c.raw_outputs()
        same_out = all(torch.equal(ra[k].view(torch.uint8) if ra[k].dtype != torch.uint8 else ra[k], outs_b[k].view(torch.uint8) if outs_b[k].dtype != torch.uint8 else outs_b[k])
                       for k in ra if torch.is_tensor(ra[k]) and k in outs_b)
        bad_out += int(not same_out)
        st_a, st_b = a.get_env_state(), b.get_env_state()
        bad_state += int(not all(torch.equal(st_a[k].view(torch.uint8), st_b[k].view(torch.uint8)) for k in st_a))
        rows = term != 0
        keep_ok = all(torch.equal(rc[k].view(torch.uint8), clone[k].view(torch.uint8)) for k in KEEP)            # respawn touched none of them
        keep_ok = keep_ok and all(torch.equal(ra[k].cpu()[rows].view(torch.uint8), clone[k].cpu()[rows].view(torch.uint8)) for k in KEEP)
        keep_ok = keep_ok and all(torch.equal(outs_c[k].view(torch.uint8), ra[k].view(torch.uint8)) for k in ("team_positions", "obs_distance", "obs_type"))
        bad_keep += int(not keep_ok)
    for e in (a, b, c):
        e.check_errors()
    cnt = sa.counters()
    for e in (a, b, c):
        e.close()
    return dict(terminal=terminal, bad_out=bad_out, bad_state=bad_state, bad_keep=bad_keep, bad_placed=bad_placed, counters=cnt)


def step_env():
    for repeat in (1, 3):
        r = run_env_pair(repeat)
        print(f"env (max_step_count 8, 24 random ticks, repeat {repeat}): {r}", flush=True)
        check(r["terminal"] > 0, f"repeat {repeat}: terminal rows occur")
        check(r["bad_out"] == 0, f"repeat {repeat}: every output buffer equals the hand-driven env's after every tick ({r['bad_out']} ticks differ)")
        check(r["bad_state"] == 0, f"repeat {repeat}: get_env_state() equals the hand-driven env's after every tick ({r['bad_state']} ticks differ)")
        check(r["bad_keep"] == 0, f"repeat {repeat}: reward, flags, winner and final_positions stay the terminal tick's ({r['bad_keep']} ticks differ)")
        check(r["bad_placed"] == 0, f"repeat {repeat}: placed.sum() equals the terminal rows on every tick: no fallback")
        c = r["counters"]
        check(c["ended"] == r["terminal"] == c["requested"] == c["placed_total"], f"repeat {repeat}: the counters add up ({c})")
    # rollout_random refuses, reset places
    env = make_env(64)
    from as_cops_and_thieves_amd.selfplay.curriculum import GeodesicSpawner
    sp = GeodesicSpawner(env, 4, 9, slots=slice(0, 40))
    env.set_spawner(sp)
    try:
        env.rollout_random(4)
        check(False, "rollout_random with a spawner raises")
    except ValueError:
        pass
    env.reset()
    d = nv.separation(env.raw_outputs()["team_positions"], sp.field, [0, 1], [0b100, 0b100]).cpu()
    check(bool(((d[:, :40] >= 4) & (d[:, :40] <= 9)).all()) and sp.reset_placed.cpu().tolist() == [1] * 40 + [0] * 24, "reset places the banded slots and no other")
    env.set_spawner(None)
    env.rollout_random(4)
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------- 3. the trainer
def make_trainer(graph, N=64, role=None, **tc):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    env = VecCopsEnv(load_preset("squarinth", 2, 1), N, num_rays=64, max_step_count=12, seed=5, final_positions=True, track_episodes=True)
    rc = RoleConfig(random_timesteps=0, learning_starts=0, **(role or {}))
    cfg = TrainerConfig(horizon=16, bptt=16, policy_freeze_duration=0, opponent_freeze_duration=0, graph_rollout=graph, episode_stats=True, **tc)
    return env, MAPPOTrainer(env, {"cop": rc, "thief": rc}, cfg, seed=2)


def collects(tr, n):
    rl = next(iter(tr.roles.values()))
    rows = []
    for _ in range(n):
        tr.collect()
        torch.cuda.synchronize()
        rows.append({k: rl.buf[k].clone() for k in ("rew", "act", "logp", "pin")} | {"done": tr._done_buf.clone()})
    return rows


def equal_rows(a, b):
    return all(torch.equal(x[k].view(torch.uint8) if x[k].dtype != torch.bool else x[k], y[k].view(torch.uint8) if y[k].dtype != torch.bool else y[k])
               for x, y in zip(a, b) for k in x)


def fresh_separations(env, tr):
    """The separations of the cops in the slots whose episode ended on the rollout's last tick: their new episode's first state."""
    fresh = tr._done_buf[-1].cpu()
    d = nv.separation(env.raw_outputs()["team_positions"], tr._spawner.field, [0, 1], [0b100, 0b100]).cpu()
    return d[:, fresh], int(fresh.sum())


def step_trainer():
    # (a trainer seeds the global generator when it is built: each is built right before its own collects)
    env_g, graph = make_trainer(True, spawn_curriculum=(2, 6))
    rows_g = collects(graph, 3)
    check(graph._graph is not None, "the second and third collects of the graph trainer run from a graph")
    check(all(bool(r["done"].any()) for r in rows_g), "episodes end in every rollout")
    # max_step_count 12 against 16-tick rollouts: the time limits fall on ticks 12, 24, 36, 48 -- the last tick of the third rollout
    d, n = fresh_separations(env_g, graph)
    check(n > 0 and bool(((d >= 2) & (d <= 6)).all()), f"after the third rollout {n} slots have just respawned, every cop 2 .. 6 hops from the thief")
    held = graph._graph
    graph._spawner.set_band(8, 12)
    collects(graph, 3)                                      # ... and on ticks 60, 72, 84, 96: the last tick of the sixth
    d, n = fresh_separations(env_g, graph)
    check(graph._graph is held, "set_band between two replays: no recapture")
    check(n > 0 and bool(((d >= 8) & (d <= 12)).all()), f"after set_band(8, 12) and three replays {n} slots have just respawned, every cop 8 .. 12 hops away")
    c = graph._spawner.counters()                           # (the trainer's first reset placed all 64 slots: requested and placed, not ended)
    check(c["ended"] > 0 and c["placed_total"] == c["requested"] == c["ended"] + 64, f"the counters followed the replays ({c})")
    env_g.close()
    env_e, eager = make_trainer(False, spawn_curriculum=(2, 6))
    rows_e = collects(eager, 3)
    check(eager._graph is None, "the graph_rollout=False trainer runs eagerly")
    check(equal_rows(rows_g, rows_e), "the rollout buffers are bit-equal: eager, captured and replayed")
    env_e.close()
    # off: nothing is built, and the trainer is the one built without the field
    env_o, off = make_trainer(True, spawn_curriculum=None, curriculum_fraction=0.5)
    rows_o = collects(off, 3)
    check(off._spawner is None and env_o._spawner is None, "off: no spawner is built or attached")
    digest = off.param_digest()
    env_o.close()
    env_p, plain = make_trainer(True)
    rows_p = collects(plain, 3)
    check(digest == plain.param_digest() and equal_rows(rows_o, rows_p), "off: param_digest and the buffers equal a trainer built without the field")
    check(not equal_rows(rows_o, rows_g), "on differs from off")
    print(f"trainer: counters {c}", flush=True)
    env_p.close()


# ---------------------------------------------------------------------------------------------- 4. win rate by initial separation
def step_separation_eval():
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_by_separation
    env = VecCopsEnv(load_preset("squarinth", 2, 1), 64, num_rays=64, max_step_count=40, seed=7)
    actor = LeagueActor.from_env(env, 3, fused="kernel")
    bands = [(2, 6), (10, 14)]
    res = evaluate_by_separation(env, actor, bands, 32, who={a: g for g, a in enumerate(env.possible_agents)})
    print({k: v for k, v in res.items()}, flush=True)
    check(set(res) == {"bands", "episodes", "cop_wins", "thief_wins", "timeouts", "cop_win_rate", "fallback_share", "ticks"}, "the table has the right keys")
    check(res["bands"] == [[2, 6], [10, 14]] and res["episodes"] == [32, 32], "two bands of 32 episodes")
    check(all(c + w + o == 32 for c, w, o in zip(res["cop_wins"], res["thief_wins"], res["timeouts"])), "the per-band episode counts add up")
    check(res["fallback_share"] == [0.0, 0.0], "no slot fell back at these bands")
    check(env._spawner is None, "the spawner is detached afterwards")
    try:
        evaluate_by_separation(env, actor, bands, 16, who={a: "random" for a in env.possible_agents})
        check(False, "a slot count that does not fit is refused")
    except ValueError:
        check(env._spawner is None, "... and nothing stays attached")
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------- 5. a short training run
def step_train():
    env, tr = make_trainer(True, role=dict(learning_epochs=1, mini_batches=2, kl_threshold=0.0), timesteps=64, spawn_curriculum=(2, 6),
                           curriculum_adapt=(0.3, 0.7), curriculum_max=20)
    with torch.enable_grad():
        tr.train(64)
    torch.cuda.synchronize()
    stats = tr.read_stats()
    cur = {k: v for k, v in stats.items() if k.startswith("curriculum/")}
    print(cur, flush=True)
    check(set(cur) == {"curriculum/hi", "curriculum/cop_win_rate", "curriculum/placed", "curriculum/fallbacks"}, "the four curriculum/* keys in read_stats()")
    check(2 <= cur["curriculum/hi"] <= 20 and cur["curriculum/placed"] > 0 and cur["curriculum/fallbacks"] == 0, "the figures are plausible")
    check(all(bool(torch.isfinite(rl.fp.master).all()) for rl in tr.roles.values()), "finite parameters after train()")
    check(tr._graph is not None, "the rollout with respawns was captured")
    check(tr.state_dict()[tr.META_KEY]["curriculum"] == {"lo": 2, "hi": tr._spawner.hi}, "state_dict carries the band")
    env.check_errors()
    env.close()


STEPS = {"synthetic": step_synthetic, "env": step_env, "trainer": step_trainer, "separation_eval": step_separation_eval, "train": step_train}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    STEPS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("FAILED CHECKS:" if FAILED else "ALL CHECKS PASSED", *FAILED, sep="\n  ", flush=True)
    sys.exit(1 if FAILED else 0)
