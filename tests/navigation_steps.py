"""The GPU steps of tests/test_gpu_navigation.py, one per process: ``python -m tests.navigation_steps STEP`` (the helpers and the conventions
of tests/act_steps.py: a step prints its figures and exits 0 when every check holds, 1 with the failed checks listed)."""
from __future__ import annotations

import sys

import numpy as np
import torch

from as_cops_and_thieves_amd import navigation as nv
from tests import navigation_cases as nc
from tests.act_steps import FAILED, check, guarded


# ---------------------------------------------------------------------------------------------- 1. the table
def step_build():
    from as_cops_and_thieves_amd.maps import load_preset
    rng = np.random.default_rng(64)
    big = ((rng.random(4096) >= 0.3).astype(np.uint8), 64, 64)
    cases = {"7x5": [nc.MASK_7X5], "1x1": [(np.ones(1, np.uint8), 1, 1)], "1x9": [(np.ones(9, np.uint8), 1, 9)], "64x64": [big],
             "13x9 free": [nc.OPEN_13X9], "two maps": [nc.MASK_7X5, nc.OPEN_13X9], "1x1 blocked": [(np.zeros(1, np.uint8), 1, 1)]}
    for name, masks in cases.items():
        field = nv.NavField(16, masks, [], device="cuda")
        torch.cuda.synchronize()
        for m, (free, Wc, Hc) in enumerate(masks):
            want = nv.hops_reference(free, Wc, Hc)
            got = field.hops_of(m)
            check(np.array_equal(got, want), f"{name}: map {m} ({Wc} x {Hc}) equals hops_reference on the whole table ({int((got != want).sum())} differ)")
            check(np.array_equal(field.snap_of(m), nv.snap_cells(free, Wc, Hc)) and np.array_equal(field.free_of(m), free), f"{name}: map {m} free and snap")
            reach = want[want != nv.NONE]
            print(f"build {name}: map {m} {Wc} x {Hc}, {int(free.sum())} free, longest path {int(reach.max()) if reach.size else -1}", flush=True)
    cm = load_preset("labyrinth").compile()
    field = nv.NavField.from_maps([cm], [], 16, 6.0, device="cuda")
    torch.cuda.synchronize()
    free, Wc, Hc = nv.free_cells(cm, 16, 6.0)
    C = Wc * Hc
    goals = np.concatenate([np.random.default_rng(7).permutation(C)[:64], [0, C - 1]])
    want, got = nv.hops_reference(free, Wc, Hc, goals), field.hops_of(0)
    check(got.shape == (C, C) and np.array_equal(got[goals], want), f"labyrinth: {len(goals)} goal rows equal hops_reference")
    check(int(free[goals].sum()) > 30 and int((1 - free[goals]).sum()) > 5, "labyrinth: the rows hold free and blocked goals")
    print(f"build labyrinth: {Wc} x {Hc}, {int(free.sum())} free, longest path on the rows {int(want[want != nv.NONE].max())}", flush=True)


# ---------------------------------------------------------------------------------------------- 2. the tick on synthetic buffers
SHARES = ("invalid", "snapped", "no snap", "unreachable", "same cell", "pursue tie", "flee tie", "flee sum tie")


def synthetic_case(A, seed):
    """(N, agents, scripts per navigator, masks, bounds, table rows, positions f32, uniform, expected actions / hops / tags per row)."""
    N = 70
    masks = [nc.MASK_7X5, nc.YARD_12X10]
    n_cops = 2 if A == 3 else 3
    agents = [2, 0] if A == 3 else [0, 1, 3, 4]                     # agent 1 (A = 3) / 2 (A = 5) is no navigator
    role = [nv.PURSUE if a < n_cops else nv.FLEE for a in agents]
    masks_opp = [sum(1 << j for j in range(A) if (j < n_cops) != (a < n_cops)) for a in agents]
    bounds = [0, 23, 47, N]
    rows = [[role[g]] * 3 for g in range(len(agents))]
    rows[0][1] = -1                                                  # the first navigator rests in the middle segment
    pos, slot_map = nc.synthetic_positions(seed, N, A, n_cops, masks)
    u = np.random.default_rng(seed + 1).random((len(agents), N)).astype(np.float32)
    return N, agents, masks_opp, masks, slot_map, bounds, rows, pos, u


def step_synthetic():
    from as_cops_and_thieves_amd import _learn_native as ln
    for A, seed in ((3, 11), (5, 12)):
        N, agents, masks_opp, masks, slot_map, bounds, rows, pos, u = synthetic_case(A, seed)
        G = len(agents)
        tables = [(f, nv.snap_cells(f, Wc, Hc), nv.hops_reference(f, Wc, Hc), Wc, Hc) for f, Wc, Hc in masks]
        # the generator's shares, by a plain per-row statement of the rule, before anything runs on the GPU
        count = {k: 0 for k in SHARES}
        want_a, want_h, live = np.full((G, N), -1), np.full((G, N), -1), 0
        for g in range(G):
            opp = [j for j in range(A) if (masks_opp[g] >> j) & 1]
            for n in range(N):
                sc = rows[g][[s for s in range(3) if bounds[s] <= n < bounds[s + 1]][0]]
                if sc < 0:
                    continue
                live += 1
                f, snap, hops, Wc, Hc = tables[slot_map[n]]
                want_a[g, n], want_h[g, n], tags = nc.rule_row(pos[n], agents[g], opp, sc, u[g, n], f, snap, hops, Wc, Hc)
                for t in tags:
                    count[t] += 1
        pursuers = sum(1 for g in range(G) for n in range(N) if rows[g][0] == nv.PURSUE and not (g == 0 and 23 <= n < 47))
        print(f"synthetic A = {A}: {live} rows, shares {count}, pursue rows {pursuers}", flush=True)
        for k in SHARES:
            of = pursuers if k == "pursue tie" else live - pursuers if k.startswith("flee") else live
            check(count[k] * 10 >= of, f"A = {A}: at least a tenth of the rows hit {k!r}: {count[k]} of {of}")
        field = nv.NavField(16, masks, slot_map, device="cuda")
        tp = torch.from_numpy(pos).to(torch.float16).cuda()
        ut = torch.from_numpy(u).cuda()
        script = torch.tensor([[rows[g][[s for s in range(3) if bounds[s] <= n < bounds[s + 1]][0]] for n in range(N)] for g in range(G)], device="cuda")
        ref_a, ref_h = nv.navigate_step(tp, ut, field, agents, script, masks_opp)
        check(np.array_equal(ref_a.cpu().numpy(), want_a) and np.array_equal(ref_h.cpu().numpy(), want_h), f"A = {A}: navigate_step equals the per-row statement")
        table = ln.nav_table(N, G, bounds, rows)
        for bound in (True, False):
            (actions, aw, band), (hops, hw, _) = guarded((N, A), torch.int32, 77), guarded((G, N), torch.int32, -9)
            actions.fill_(9); hops.fill_(-5)
            before = tp.clone()
            ln.nav_step(tp, ut, field, agents, masks_opp, table, actions, hops if bound else None)
            torch.cuda.synchronize()
            on = script >= 0
            cols = actions[:, torch.tensor(agents, device="cuda")].t()
            check(torch.equal(cols[on], ref_a[on]), f"A = {A} nav_hops {'bound' if bound else 'NULL'}: actions equal navigate_step ({int((cols[on] != ref_a[on]).sum())} differ)")
            check(bool((cols[~on] == 9).all()), f"A = {A}: the column of a navigator with script -1 keeps its sentinel")
            others = [j for j in range(A) if j not in agents]
            check(bool((actions[:, others] == 9).all()), f"A = {A}: the columns of agents that are no navigators keep their sentinel")
            if bound:
                check(torch.equal(hops[on], ref_h[on]) and bool((hops[~on] == -5).all()), f"A = {A}: nav_hops equals navigate_step, -1 rows untouched")
            else:
                check(bool((hops == -5).all()), f"A = {A}: a NULL nav_hops writes nothing")
            for w, fill, name in ((aw, 77, "actions"), (hw, -9, "nav_hops")):
                ref = torch.full((band,), fill, dtype=w.dtype, device="cuda")
                check(torch.equal(w[:band], ref) and torch.equal(w[-band:], ref), f"A = {A}: guard bands of {name} intact")
            check(torch.equal(tp.view(torch.int16), before.view(torch.int16)), "the positions are not written")


# ---------------------------------------------------------------------------------------------- 3. on an env
def make_env(name="labyrinth", N=64, msc=100, seed=3, **kw):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    env = VecCopsEnv(load_preset(name, 2, 1), N, num_rays=64, max_step_count=msc, seed=seed, **kw)
    env.reset()
    return env


WHO = {"cop_0": "pursue", "cop_1": "pursue", "thief_0": "flee"}


def step_env():
    from as_cops_and_thieves_amd.selfplay.navigators import NavigatorActor
    N, T = 64, 200
    env = make_env()
    actor = NavigatorActor(env, WHO)
    check(actor.fused and actor.indices == [0, 1, 2] and actor.opponent_masks == [0b100, 0b100, 0b011], "a fused actor over all three agents")
    script = torch.tensor([[0], [0], [1]], device="cuda").expand(3, N)
    bad_a = torch.zeros((), dtype=torch.int64, device="cuda")
    bad_h, ends, fallbacks, hop_sum = bad_a.clone(), bad_a.clone(), bad_a.clone(), bad_a.clone()
    seen = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.manual_seed(6)
    for t in range(T):
        u = torch.rand(3, N, device="cuda")
        want, hops = nv.navigate_step(env.raw_outputs()["team_positions"], u, actor.field, actor.indices, script, actor.opponent_masks)
        actions = actor.act(env, uniform=u)
        bad_a += (actions.t() != want).sum()
        bad_h += (actor.nav_hops != hops).sum()
        fallbacks += (hops < 0).sum()
        hop_sum += hops.clamp(min=0).sum()
        seen += torch.bincount(actions.flatten().long(), minlength=4)[:4]
        ends += (env.step_raw(actions)["terminated"] != 0).sum()
    print(f"env: {int(ends)} episodes ended, {int(fallbacks)} fallback rows of {3 * N * T}, mean hops {int(hop_sum) / (3 * N * T):.2f}, actions {seen.tolist()}", flush=True)
    check(int(bad_a) == 0, f"actions equal navigate_step on all {T} ticks ({int(bad_a)} differ)")
    check(int(bad_h) == 0, f"nav_hops equal navigate_step on all {T} ticks ({int(bad_h)} differ)")
    # (the labyrinth has no wall along its border: an agent that leaves the window has no cell and its row falls back, so fallback rows are
    # part of the comparison above, not an error)
    check(int(ends) > 0 and bool((seen > 0).all()) and 0 < int(fallbacks) < 3 * N * T, "episodes end, all four actions occur, rule and fallback rows both occur")
    env.check_errors()
    check(True, "device_errors 0")
    env.close()


# ---------------------------------------------------------------------------------------------- 4. captured
def step_graph():
    from as_cops_and_thieves_amd.selfplay.navigators import NavigatorActor
    N, T = 64, 20
    torch.manual_seed(8)
    us = torch.rand(T + 1, 3, N, device="cuda")
    runs = {}
    for captured in (False, True):
        env = make_env()
        actor = NavigatorActor(env, WHO)
        u, log, hop_log = torch.zeros(3, N, device="cuda"), [], []
        tick = lambda: env.step_raw(actor.act(env, uniform=u))
        u.copy_(us[T])
        tick()                                              # one eager tick in both runs: every op has run once before the capture
        if captured:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                   # (recorded, not run)
                tick()
            tick = graph.replay
        for t in range(T):
            u.copy_(us[t])
            tick()
            log.append(actor.actions.clone()); hop_log.append(actor.nav_hops.clone())
        torch.cuda.synchronize()
        runs[captured] = (torch.stack(log), torch.stack(hop_log), env.raw_outputs()["team_positions"].clone())
        env.check_errors()
        env.close()
    (a0, h0, p0), (a1, h1, p1) = runs[False], runs[True]
    check(torch.equal(a0, a1) and torch.equal(h0, h1), f"the replayed ticks give the eager loop's actions and hops ({int((a0 != a1).sum())} differ)")
    check(torch.equal(p0.view(torch.int16), p1.view(torch.int16)), "and the same positions after 20 ticks")
    check(len({tuple(x.flatten().tolist()) for x in a0}) > 10, "the actions move from tick to tick")


# ---------------------------------------------------------------------------------------------- 5. MAPPOTrainer.set_opponent
def step_opponent():
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    from as_cops_and_thieves_amd.selfplay.navigators import NavigatorActor
    N, T = 64, 16
    shots = {}
    for graph in (False, True):
        env = make_env("squarinth", N, 40)
        rc = lambda: RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0, kl_threshold=0.0)
        tcfg = TrainerConfig(horizon=T, bptt=T, policy_freeze_duration=0, opponent_freeze_duration=0, graph_rollout=graph, graph_update=False)
        tr = MAPPOTrainer(env, {"cop": rc(), "thief": rc()}, tcfg, seed=4, split_roles=True)
        actor = NavigatorActor(env, {"thief_0": "flee"})
        tr.set_opponent("thief", actor)
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        ticks = []
        if not graph:                                       # the eager twin: every tick of every rollout is held against the rule
            act = actor.act

            def checked(env_, starts=None, obs=None, actions=None, uniform=None):
                u = torch.rand(1, N, device="cuda")
                want, _ = nv.navigate_step(env_.raw_outputs()["team_positions"], u, actor.field, actor.indices, [nv.FLEE], actor.opponent_masks)
                out = act(env_, starts, obs=obs, actions=actions, uniform=u)
                bad.add_((out[:, 2] != want[0]).sum())
                ticks.append(1)
                return out

            actor.act = checked
        torch.manual_seed(77)
        snaps = []
        for i in range(3):
            tr.collect()
            torch.cuda.synchronize()
            cop = tr.roles["cop"]
            snaps.append(dict({k: cop.buf[k].clone() for k in ("act", "logp", "rew")}, done=tr._done_buf.clone(), actions=tr._actions.clone()))
        shots[graph] = snaps
        if graph:
            check(tr._graph is not None, "the rollout with a NavigatorActor is one captured graph")
        else:
            check(tr._graph is None and len(ticks) == 3 * T and int(bad) == 0, f"eager twin: the thief column is the rule on all {len(ticks)} ticks ({int(bad)} differ)")
        check(not any(bool(v.any()) for v in tr.roles["thief"].buf.values()), "no rollout row of the thieves is kept")
        env.check_errors()
        env.close()
    for i in range(3):
        for k in shots[False][i]:
            check(torch.equal(shots[False][i][k], shots[True][i][k]), f"rollout {i}: {k} of the captured trainer equals the eager twin's")
    check(any(bool(s["done"].any()) for s in shots[True]), "episodes end inside the rollouts")


# ---------------------------------------------------------------------------------------------- 6. the callers
def step_users():
    """``evaluate_against_navigators`` without and with learned policies, and ``watch(navigators=...)``."""
    import json
    import tempfile
    from pathlib import Path
    from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
    from as_cops_and_thieves_amd.selfplay.self_play import NAVIGATOR_MATCHUPS, evaluate_against_navigators
    from as_cops_and_thieves_amd.selfplay.watch import watch
    E = 16
    env = make_env("squarinth", E, 40, seed=11)
    torch.manual_seed(12)
    res = evaluate_against_navigators(env, None, E)
    check(res["segments"] == [n for n in NAVIGATOR_MATCHUPS if "cops" not in n and "thieves" not in n] and len(res["segments"]) == 5, "source=None skips the learned rows")
    trainer = MAPPOTrainer(env, {"cop": CFG_AGENT, "thief": CFG_AGENT}, TrainerConfig(graph_rollout=False, graph_update=False), seed=2)
    full = evaluate_against_navigators(env, trainer, E)
    check(full["segments"] == list(NAVIGATOR_MATCHUPS), "a trainer as the source plays all seven match-ups")
    for r in (res, full):
        check(all(c + t + o == E for c, t, o in zip(r["cop_wins"], r["thief_wins"], r["timeouts"])), "every slot's first episode is counted once")
        check(all(h is not None and 0 <= h < 4000 for h in r["mean_hops"]) and all(0 < m <= 40 for m in r["mean_length"]), "mean hops and lengths are in range")
        print("users:", {n: (c, round(h, 1)) for n, c, h in zip(r["segments"], r["cop_wins"], r["mean_hops"])}, flush=True)
    try:
        evaluate_against_navigators(env, None, E + 1)
        check(False, "an env of another size is refused")
    except ValueError:
        pass
    env.check_errors()
    env.close()
    with tempfile.TemporaryDirectory() as tmp:
        who = {"cop": "pursue", "thief": "flee"}
        out = watch("squarinth", 2, Path(tmp), ticks=12, seed=3, max_step_count=400, fused_act=True, navigators=who, log=lambda *a: None)
        book = json.loads((Path(tmp) / "episode.json").read_text())
        check(book["navigators"] == who and out["navigators"] == who and len(out["slots"]) == 2 and len(list((Path(tmp) / "env_0").glob("frame_*.png"))) >= 2,
              "watch plays navigator roles: clips and book")
        for bad in ({"cop": "flee"}, {"robber": "pursue"}):
            try:
                watch("squarinth", 2, Path(tmp) / "bad", ticks=2, fused_act=True, navigators=bad, log=lambda *a: None)
                check(False, f"watch refuses {bad}")
            except ValueError:
                pass


STEPS = {"build": step_build, "synthetic": step_synthetic, "env": step_env, "graph": step_graph, "opponent": step_opponent, "users": step_users}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    STEPS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("FAILED CHECKS:" if FAILED else "ALL CHECKS PASSED", *FAILED, sep="\n  ", flush=True)
    sys.exit(1 if FAILED else 0)
