"""The GPU steps of tests/test_gpu_scripted.py, one per process: ``python -m tests.scripted_steps STEP`` (the helpers and the conventions of
tests/act_steps.py: a step prints its figures and exits 0 when every check holds, 1 with the failed checks listed)."""
from __future__ import annotations

import sys

import torch

from tests import scripted_cases as sc
from tests.act_steps import FAILED, check, guarded

SHAPES = ((1, 2, 2, 8), (67, 3, 3, 64), (33, 5, 5, 90), (5, 3, 2, 300))          # (N, A, G, R)


def setup(N, A, G, R, bounds=None, scripts=None):
    """(agent map, targets, table) of a launch: G = 2 takes a non-identity agent map."""
    from as_cops_and_thieves_amd import _learn_native as ln
    agent = [A - 1, 0] if G == 2 else list(range(G))
    target = [sc.THIEF if g % 2 == 0 else sc.COP for g in range(G)]
    bounds = [0, N] if bounds is None else bounds
    scripts = [[g % 2] * (len(bounds) - 1) for g in range(G)] if scripts is None else scripts
    return agent, target, ln.scripted_table(N, G, bounds, scripts)


def launch(od, ot, agent, target, table, u, keep, state, actions, params=sc.DEFAULT):
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.rollout_scripted({"obs_distance": od, "obs_type": ot}, agent, target, table, u, keep, state, actions, params.memory_ticks, params.clear_min,
                        params.turn_prob)


def torch_form(od, ot, agent, target, table, u, keep, state, params=sc.DEFAULT):
    """(actions [G, N] with -1 where not scripted, new state [G, N, 4]) by ``scripted_step`` on the same buffers."""
    from as_cops_and_thieves_amd.selfplay.scripted import scripted_step
    G, N = u.shape
    script = torch.empty(G, N, dtype=torch.int64)
    for s, (lo, hi) in enumerate(zip(table.start[:-1], table.start[1:])):
        for g in range(G):
            script[g, lo:hi] = table.rows[g][s]
    idx = torch.tensor(agent, device=od.device)
    d, t = od[:, idx].transpose(0, 1).contiguous(), ot[:, idx].transpose(0, 1).contiguous()
    return scripted_step(d, t, u, state, None if keep is None else keep.view(1, N), script.to(od.device), torch.tensor(target, device=od.device).view(G, 1),
                         params)


def columns(actions, agent):
    return actions[:, torch.tensor(agent, device=actions.device)].t()          # [G, N]


# ---------------------------------------------------------------------------------------------- 1. the hand cases through the kernel
def step_hand():
    from as_cops_and_thieves_amd import _learn_native as ln
    for c in sc.HAND_CASES:
        d, t, u, state, keep = sc.case_tensors(c, "cuda")
        od, ot = d.view(1, 1, 8).contiguous(), t.view(1, 1, 8).contiguous()
        st = state.view(1, 1, 4).clone()
        actions = torch.full((1, 1), 9, dtype=torch.int32, device="cuda")
        launch(od, ot, [0], [c["target"]], ln.scripted_table(1, 1, [0, 1], [[c["script"]]]), u.view(1, 1), None if keep is None else keep.view(1), st, actions,
               c["params"])
        check(int(actions) == c["action"] and tuple(st.view(4).tolist()) == c["new_state"], f"{c['name']}: {int(actions)} {st.view(4).tolist()}")
    print("hand cases:", len(sc.HAND_CASES), flush=True)


# ---------------------------------------------------------------------------------------------- 2. against the torch form
def step_random():
    from as_cops_and_thieves_amd.selfplay.scripted import ScriptedParams
    for i, (N, A, G, R) in enumerate(SHAPES):
        agent, target, table = setup(N, A, G, R)
        params = sc.DEFAULT if i % 2 == 0 else ScriptedParams(memory_ticks=1, clear_min=20.0, turn_prob=0.3)
        gen = torch.Generator(device="cuda").manual_seed(N + R)
        state_k = torch.zeros(G, N, 4, dtype=torch.int32, device="cuda")
        state_t = state_k.clone()
        sees = blocked = 0
        for tick in range(3):
            od, ot = sc.random_buffers(N, A, R, seed=100 * tick + N, device="cuda")
            u = torch.rand(G, N, generator=gen, device="cuda")
            keep = None if tick == 0 else (torch.rand(N, generator=gen, device="cuda") < (0.5 if tick == 1 else 0.9)).float()
            actions = torch.full((N, A), 9, dtype=torch.int32, device="cuda")
            launch(od, ot, agent, target, table, u, keep, state_k, actions, params)
            want, state_t = torch_form(od, ot, agent, target, table, u, keep, state_t, params)
            check(torch.equal(columns(actions, agent), want), f"actions {(N, A, G, R)} tick {tick}")
            check(torch.equal(state_k, state_t), f"state {(N, A, G, R)} tick {tick}")
            idx = torch.tensor(agent, device="cuda")
            sees += int((ot[:, idx] == torch.tensor(target, device="cuda").view(1, G, 1)).any(-1).sum())
            blocked += int((od[:, idx].float().max(-1).values < params.clear_min).sum())
        print(f"{(N, A, G, R)}: rows that see their target {sees}/{3 * G * N}, with every cone blocked {blocked}/{3 * G * N}", flush=True)
        if N > 30:
            check(0.15 < sees / (3 * G * N) < 0.5 and blocked > 0, f"the buffers exercise sight and blocked fans {(N, A, G, R)}")
        check(bool((state_k[..., 0] == 1).all()) and bool(((state_k[..., 1] >= 0) & (state_k[..., 1] <= 3)).all()), f"state rows are valid {(N, A, G, R)}")


# ---------------------------------------------------------------------------------------------- 3. untouched memory
def step_untouched():
    N, A, G, R = 37, 4, 2, 90
    from as_cops_and_thieves_amd import _learn_native as ln
    agent, target = [3, 1], [sc.THIEF, sc.COP]
    bounds, scripts = [0, 5, 20, 37], [[0, -1, 0], [-1, 1, -1]]
    table = ln.scripted_table(N, G, bounds, scripts)
    od0, ot0 = sc.random_buffers(N, A, R, seed=5, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    (od, odw, b), (ot, otw, _) = guarded((N, A, R), torch.float16, 123.0), guarded((N, A, R), torch.uint8, 7)
    (u, uw, _), (keep, kw, _) = guarded((G, N), torch.float32, -2.0), guarded((N,), torch.float32, -2.0)
    (state, sw, _), (actions, aw, _) = guarded((G, N, 4), torch.int32, -7), guarded((N, A), torch.int32, 77)
    od.copy_(od0); ot.copy_(ot0)
    u.copy_(torch.rand(G, N, generator=gen, device="cuda"))
    keep.copy_((torch.rand(N, generator=gen, device="cuda") < 0.7).float())
    state0 = torch.randint(0, 4, (G, N, 4), generator=gen, device="cuda", dtype=torch.int32)
    state.copy_(state0)
    actions.fill_(9)
    inputs = [t.clone() for t in (od, ot, u, keep)]
    launch(od, ot, agent, target, table, u, keep, state, actions)
    torch.cuda.synchronize()
    for w, fill, name in ((odw, 123.0, "obs_distance"), (otw, 7, "obs_type"), (uw, -2.0, "uniform"), (kw, -2.0, "keep"), (sw, -7, "state"), (aw, 77, "actions")):
        ref = torch.full((b,), fill, dtype=w.dtype, device="cuda")
        check(torch.equal(w[:b], ref) and torch.equal(w[-b:], ref), f"guard bands of {name} intact")
    check(all(torch.equal(x, y) for x, y in zip(inputs, (od, ot, u, keep))), "the inputs are not written")
    check(bool((actions[:, [0, 2]] == 9).all()), "columns of agents the launch does not cover keep their sentinel")
    want, new = torch_form(od, ot, agent, target, table, u, keep, state0)
    for g in range(G):
        for s in range(3):
            lo, hi = bounds[s], bounds[s + 1]
            if scripts[g][s] < 0:
                check(bool((actions[lo:hi, agent[g]] == 9).all()) and torch.equal(state[g, lo:hi], state0[g, lo:hi]), f"policy {g} segment {s}: -1 rows untouched")
            else:
                check(torch.equal(actions[lo:hi, agent[g]], want[g, lo:hi]) and torch.equal(state[g, lo:hi], new[g, lo:hi]), f"policy {g} segment {s}: the rule")
                check(bool((state[g, lo:hi, 0] == 1).all()), f"policy {g} segment {s}: state written")


# ---------------------------------------------------------------------------------------------- 4. segment tables
def step_segments():
    N, A, G, R = 67, 3, 3, 64
    bounds = [0, 3, 40, 67]
    scripts = [[0, 1, 0], [1, -1, 1], [-1, 0, 1]]
    agent, target, table = setup(N, A, G, R, bounds, scripts)
    od, ot = sc.random_buffers(N, A, R, seed=8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(2)
    u = torch.rand(G, N, generator=gen, device="cuda")
    keep = (torch.rand(N, generator=gen, device="cuda") < 0.7).float()
    state0 = torch.randint(0, 4, (G, N, 4), generator=gen, device="cuda", dtype=torch.int32)
    state0[..., 2] = torch.randint(0, R, (G, N), generator=gen, device="cuda", dtype=torch.int32)
    state, actions = state0.clone(), torch.full((N, A), 9, dtype=torch.int32, device="cuda")
    launch(od, ot, agent, target, table, u, keep, state, actions)
    for s in range(3):
        lo, hi = bounds[s], bounds[s + 1]
        _, _, one = setup(hi - lo, A, G, R, [0, hi - lo], [[row[s]] for row in scripts])
        st, ac = state0[:, lo:hi].contiguous(), torch.full((hi - lo, A), 9, dtype=torch.int32, device="cuda")
        launch(od[lo:hi], ot[lo:hi], agent, target, one, u[:, lo:hi].contiguous(), keep[lo:hi].contiguous(), st, ac)
        check(torch.equal(actions[lo:hi], ac) and torch.equal(state[:, lo:hi], st), f"segment {s} = the S = 1 launch on rows [{lo}, {hi})")
    check(bool((actions != 9).any()) and bool((actions == 9).any()), "scripted and unscripted cells both occur")


# ---------------------------------------------------------------------------------------------- 5. graph capture
def step_graph():
    N, A, G, R = 67, 3, 3, 64
    agent, target, table = setup(N, A, G, R, [0, 30, 67], [[0, 1], [1, -1], [1, 0]])
    od, ot = sc.random_buffers(N, A, R, seed=3, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(4)
    u = torch.rand(G, N, generator=gen, device="cuda")
    keep = (torch.rand(N, generator=gen, device="cuda") < 0.7).float()
    state0 = torch.randint(0, 4, (G, N, 4), generator=gen, device="cuda", dtype=torch.int32)
    state, actions = state0.clone(), torch.full((N, A), 9, dtype=torch.int32, device="cuda")
    launch(od, ot, agent, target, table, u, keep, state, actions)
    torch.cuda.synchronize()
    eager = (actions.clone(), state.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # the launch goes to the capturing stream: _learn_native._stream()
        launch(od, ot, agent, target, table, u, keep, state, actions)
    for rep in range(2):
        state.copy_(state0); actions.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        check(torch.equal(actions, eager[0]) and torch.equal(state, eager[1]), f"replay {rep} = the eager launch")
    check(not torch.equal(eager[1], state0), "the launch moved the state")


# ---------------------------------------------------------------------------------------------- 6. on an env
def step_env():
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.scripted import ScriptedActor
    N, R, T = 64, 64, 200
    env = VecCopsEnv(load_preset("squarinth", 2, 1), N, num_rays=R, max_step_count=100, seed=3)
    env.reset()
    actor = ScriptedActor(env, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"})
    check(actor.fused and actor.targets == [2, 2, 1] and actor.indices == [0, 1, 2], "a fused actor over all three agents")
    starts = torch.ones(N, dtype=torch.bool, device="cuda")
    state_t = torch.zeros(3, N, 4, dtype=torch.int32, device="cuda")
    bad_a = torch.zeros((), dtype=torch.int64, device="cuda")
    bad_s, ends, sightings = bad_a.clone(), bad_a.clone(), bad_a.clone()
    seen = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.manual_seed(6)
    for t in range(T):
        raw = env.raw_outputs()
        u = torch.rand(3, N, device="cuda")
        want, state_t = torch_form(raw["obs_distance"], raw["obs_type"], actor.indices, actor.targets, actor.table, u, (~starts).float(), state_t)
        actions = actor.act(env, starts, uniform=u)
        bad_a += (actions.t() != want).sum()
        bad_s += (actor.state != state_t).sum()
        sightings += (state_t[..., 3] == 30).sum()
        seen += torch.bincount(actions.flatten().long(), minlength=4)[:4]
        out = env.step_raw(actions)
        torch.ne(out["terminated"], 0, out=starts)
        ends += starts.sum()
    print(f"env: {int(ends)} episodes ended, {int(sightings)} sightings, actions {seen.tolist()}", flush=True)
    check(int(bad_a) == 0, f"actions equal the torch form on all {T} ticks ({int(bad_a)} differ)")
    check(int(bad_s) == 0, f"states equal the torch form on all {T} ticks ({int(bad_s)} differ)")
    check(int(ends) > 0 and int(sightings) > 0 and bool((seen > 0).all()), "episodes end, targets are seen and all four actions occur")
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------- 7. a mixed league
def step_league():
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
    from as_cops_and_thieves_amd.selfplay.scripted import SCRIPTS
    from tests.act_steps import same
    N, R = 48, 64
    agents = ["cop_0", "cop_1", "thief_0"]
    mixed = [(0, 10, {"cop_0": 0, "cop_1": 1, "thief_0": "evade"}), (10, 31, {"cop_0": "chase", "cop_1": "random", "thief_0": 2}),
             (31, 40, {"cop_0": 1, "cop_1": 0, "thief_0": 2}), (40, 48, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"})]
    plain = [(lo, hi, {a: "random" if v in SCRIPTS else v for a, v in who.items()}) for lo, hi, who in mixed]
    env = VecCopsEnv(load_preset("squarinth", 2, 1), N, num_rays=R, max_step_count=100, seed=3)
    env.reset()
    for t in range(5):
        env.step(env.random_actions(t))
    gen = torch.Generator(device="cuda").manual_seed(7)
    h0 = torch.randn(1, 3, N, 128, generator=gen, device="cuda").mul(0.5).to(torch.bfloat16)
    c0 = torch.randn(1, 3, N, 128, generator=gen, device="cuda").to(torch.bfloat16)
    starts = torch.rand(N, generator=gen, device="cuda") < 0.3
    runs = {}
    for name, table in (("mixed", mixed), ("plain", plain)):
        actor = LeagueActor.from_env(env, 3, fused=True, seed=4)
        check(actor.fused, "the league actor is fused")
        actor.set_matchups(table)
        (key,) = actor.state
        actor.set_state({key: (h0, c0)})
        torch.manual_seed(11)
        logits = torch.zeros(3, N, 4, dtype=torch.bfloat16, device="cuda")
        acts = [actor.act(env, starts if i == 0 else None, logits_out=logits).clone() for i in range(3)]
        runs[name] = (actor, acts, logits, actor.state[key])
    (actor, acts, logits, (h, c)), (other, base, logits_b, (hb, cb)) = runs["mixed"], runs["plain"]
    check(other.script_table is None and other.script_state is None and actor.script_table is not None, "only the mixed table makes a scripted launch")
    for lo, hi, who in mixed:
        for g, a in enumerate(agents):
            cell = f"{a} rows [{lo}, {hi}) {who[a]}"
            if isinstance(who[a], int):
                check(all(torch.equal(x[lo:hi, g], y[lo:hi, g]) for x, y in zip(acts, base)), f"network cell: actions of three ticks {cell}")
                check(same(h[0, g, lo:hi], hb[0, g, lo:hi]) and same(c[0, g, lo:hi], cb[0, g, lo:hi]) and same(logits[g, lo:hi], logits_b[g, lo:hi]),
                      f"network cell: h, c and logits {cell}")
                check(bool((actor.script_state[g, lo:hi] == 0).all()), f"network cell: no scripted state {cell}")
            else:
                check(same(h[0, g, lo:hi], h0[0, g, lo:hi]) and same(c[0, g, lo:hi], c0[0, g, lo:hi]), f"recurrent rows untouched {cell}")
    # the scripted cells are the rule, from the tick's one torch.rand(G, N)
    torch.manual_seed(11)
    raw = env.raw_outputs()
    state_t = torch.zeros(3, N, 4, dtype=torch.int32, device="cuda")
    for i in range(3):
        u = torch.rand(3, N, device="cuda")
        want, state_t = torch_form(raw["obs_distance"], raw["obs_type"], [0, 1, 2], [2, 2, 1], actor.script_table, u,
                                   (~starts).float() if i == 0 else None, state_t)
        on = want >= 0
        check(torch.equal(acts[i].t()[on], want[on]), f"scripted cells: actions of tick {i}")
        rnd = torch.tensor([[who[a] == "random" for a in agents] for lo, hi, who in mixed for _ in range(lo, hi)], device="cuda").t()
        check(torch.equal(acts[i].t()[rnd], (4.0 * u).to(torch.int32).clamp(max=3)[rnd]), f"random cells stay min(3, int(4u)) on tick {i}")
    check(torch.equal(actor.script_state, state_t), "scripted cells: state after three ticks")
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------- 8. the purpose
def step_purpose():
    """Chase cops beat random cops against the same random thieves, and random cops do worse against evade thieves than against random ones:
    first episodes of 256 slots per match-up, squarinth 2v1, 64 rays, max_step_count 400, fixed seeds."""
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_league
    E = 256
    env = VecCopsEnv(load_preset("squarinth", 2, 1), 4 * E, num_rays=64, max_step_count=400, seed=11)
    actor = LeagueActor.from_env(env, 1, fused=True)
    names = ("chase v random", "random v random", "random v evade", "chase v evade")
    who = [{"cop_0": "chase", "cop_1": "chase", "thief_0": "random"}, {"cop_0": "random", "cop_1": "random", "thief_0": "random"},
           {"cop_0": "random", "cop_1": "random", "thief_0": "evade"}, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"}]
    actor.set_matchups([(s * E, (s + 1) * E, w) for s, w in enumerate(who)])
    torch.manual_seed(12)
    res = evaluate_league(env, actor)
    wins = res["cop_wins"]
    for s, n in enumerate(names):
        print(f"purpose: {n}: cop wins {wins[s]}/{E} = {wins[s] / E:.3f}, thief wins {res['thief_wins'][s]}, timeouts {res['timeouts'][s]}, "
              f"mean length {float(res['length'][s * E:(s + 1) * E].float().mean()):.1f}", flush=True)
    check(all(c + t + o == E for c, t, o in zip(wins, res["thief_wins"], res["timeouts"])), "every slot's first episode is counted")
    check(wins[0] > wins[1], f"chase cops win more episodes against random thieves than random cops do: {wins[0]} v {wins[1]}")
    check(wins[1] > wins[2], f"random cops win more episodes against random thieves than against evade thieves: {wins[1]} v {wins[2]}")
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------- 9. watch --script
def step_watch():
    import json
    import tempfile
    from pathlib import Path
    from as_cops_and_thieves_amd.selfplay.watch import watch
    with tempfile.TemporaryDirectory() as tmp:
        res = {}
        for fused in (False, True):
            out = Path(tmp) / str(fused)
            res[fused] = watch("squarinth", 2, out, ticks=12, seed=3, max_step_count=400, fused_act=fused, scripts={"cop": "chase", "thief": "evade"},
                               log=lambda *a: None)
            book = json.loads((out / "episode.json").read_text())
            check(book["scripts"] == {"cop": "chase", "thief": "evade"} and len(list((out / "env_0").glob("frame_*.png"))) >= 2, f"watch fused_act={fused}: clips and book")
        check(all(len(r["slots"]) == 2 and r["scripts"] == {"cop": "chase", "thief": "evade"} for r in res.values()), "two slots each")


STEPS = {"hand": step_hand, "random": step_random, "untouched": step_untouched, "segments": step_segments, "graph": step_graph, "env": step_env,
         "league": step_league, "purpose": step_purpose, "watch": step_watch}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    STEPS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("FAILED CHECKS:" if FAILED else "ALL CHECKS PASSED", *FAILED, sep="\n  ", flush=True)
    sys.exit(1 if FAILED else 0)
