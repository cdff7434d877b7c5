"""The GPU steps of tests/test_gpu_fused_collect.py, one per process: ``python -m tests.collect_steps STEP``.  A step prints its figures and
exits 0 when every check holds, 1 with the failed checks listed otherwise (the pattern of tests/act_steps.py)."""
from __future__ import annotations

import sys

import torch

from tests.act_steps import FAILED, check, same

NAN = float("nan")


def env_of(roster, N, R, msc, seed=3, warm=0, **kw):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    env = VecCopsEnv(load_preset("squarinth", *roster), N, num_rays=R, max_step_count=msc, seed=seed, **kw)
    env.reset()
    for t in range(warm):
        env.step(env.random_actions(t))
    return env


def twin_of(env, roster, N, R, msc, seed=3):
    """A second env in the state of ``env``: simulator state and the output buffers the next act tick reads."""
    twin = env_of(roster, N, R, msc, seed)
    twin.set_env_state(**env.get_env_state())
    src, dst = env.raw_outputs(), twin.raw_outputs()
    for k in dst:
        if k in src and isinstance(dst[k], torch.Tensor):
            dst[k].copy_(src[k])
    torch.cuda.synchronize()
    return twin


def rc(**kw):
    from as_cops_and_thieves_amd.selfplay.mappo import RoleConfig
    return RoleConfig(**{**dict(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0, kl_threshold=0.0), **kw})


# ---------------------------------------------------------------------------------------------- 1. the kernel against cat_act_step + cat_rollout_pack
def step_kernel():
    from as_cops_and_thieves_amd import _learn_native as ln
    from as_cops_and_thieves_amd.selfplay.actor import PolicyActor
    for roster, R, N in (((2, 1), 64, 70), ((1, 1), 90, 33)):
        env = env_of(roster, N, R, msc=200, warm=3)
        actor = PolicyActor.from_checkpoint(None, env, fused=True, seed=3)
        (grp,) = actor.groups.values()
        G, A, n_cops = grp.G, len(actor.agents), roster[0]
        gen = torch.Generator(device="cuda").manual_seed(N + R)
        grp.fp.lp.copy_(torch.randn(grp.fp.lp.shape, generator=gen, device="cuda").mul(0.05).to(torch.bfloat16))      # random bf16 parameters
        p = ln.act_params({n: grp.policy.w(n) for n in ln.ACT_PARAM_NAMES})
        raw = env.raw_outputs()
        TAIL = 5                                                 # sentinel rows behind the [G, N, 128] blocks of h and c
        h = torch.randn(G, N, 128, generator=gen, device="cuda").mul(0.5).to(torch.bfloat16)
        c = torch.randn(G, N, 128, generator=gen, device="cuda").to(torch.bfloat16)
        u = torch.rand(G, N, generator=gen, device="cuda")
        keep = (torch.rand(N, generator=gen, device="cuda") < 0.7).float()
        check(0 < int(keep.sum()) < N, f"keep holds zeros and ones R={R}")
        for q11 in (False, True):
            # the reference: two launches of existing entries on cloned inputs
            h_ref, c_ref = h.clone(), c.clone()
            acts_ref = torch.full((N, A), 9, dtype=torch.int32, device="cuda")
            lo_ref = torch.zeros(G, N, 4, dtype=torch.bfloat16, device="cuda")
            lp_ref = torch.zeros(G, N, device="cuda")
            ln.act_step(raw, grp.indices, p, h_ref, c_ref, keep, u, acts_ref, logits_out=lo_ref, logp_out=lp_ref, row_tile=32)
            pin_ref = torch.zeros(G, N, 2 * R, dtype=torch.bfloat16, device="cuda")
            vin_ref = torch.zeros(G, N, 4 * R, dtype=torch.bfloat16, device="cuda")
            ln.rollout_pack(raw, grp.indices, n_cops, q11, 1.0, 1.0, pin_ref, vin_ref)
            torch.cuda.synchronize()
            for tile in (32, 64):
                for with_state_out in (True, False):
                    tag = f"R={R} N={N} q11={q11} tile={tile} state_out={with_state_out}"
                    hh = torch.full((G * N + TAIL, 128), NAN, dtype=torch.bfloat16, device="cuda")
                    cc = torch.full((G * N + TAIL, 128), NAN, dtype=torch.bfloat16, device="cuda")
                    hv, cv = hh[:G * N].view(G, N, 128), cc[:G * N].view(G, N, 128)
                    hv.copy_(h); cv.copy_(c)
                    h_before, c_before = hv.clone(), cv.clone()
                    pin = torch.full((G, 3, N, 2 * R), NAN, dtype=torch.bfloat16, device="cuda")
                    vin = torch.full((G, 3, N, 4 * R), NAN, dtype=torch.bfloat16, device="cuda")
                    act = torch.full((G, 3, N), -7, dtype=torch.int64, device="cuda")
                    logp = torch.full((G, 3, N), NAN, device="cuda")
                    h0 = torch.full((G, N, 128), NAN, dtype=torch.bfloat16, device="cuda") if with_state_out else None
                    c0 = torch.full((G, N, 128), NAN, dtype=torch.bfloat16, device="cuda") if with_state_out else None
                    acts = torch.full((N, A), 9, dtype=torch.int32, device="cuda")
                    lo = torch.zeros(G, N, 4, dtype=torch.bfloat16, device="cuda")
                    lp = torch.zeros(G, N, device="cuda")
                    ln.act_collect_step(raw, grp.indices, p, hv, cv, keep, u, acts, n_cops, q11, pin[:, 1], vin[:, 1], act[:, 1], logp[:, 1], h0, c0,
                                        logits_out=lo, base_logp_out=lp, row_tile=tile)
                    torch.cuda.synchronize()
                    check(torch.equal(acts, acts_ref), f"actions {tag}")
                    check(same(hv, h_ref) and same(cv, c_ref), f"h and c {tag}")
                    check(same(lo, lo_ref) and same(lp, lp_ref), f"base logits_out / logp_out {tag}")
                    check(same(logp[:, 1], lp_ref), f"strided logp {tag}")
                    check(torch.equal(act[:, 1], acts_ref.t().long()[grp.indices]), f"act_out {tag}")
                    check(same(pin[:, 1], pin_ref), f"pin rows {tag}")
                    check(same(vin[:, 1], vin_ref), f"vin rows {tag}")
                    if with_state_out:
                        check(same(h0, h_before) and same(c0, c_before), f"h0_out / c0_out hold the state before the tick, keep not applied {tag}")
                    for name, t in (("pin", pin), ("vin", vin), ("logp", logp)):
                        check(bool(torch.isnan(t[:, 0].float()).all()) and bool(torch.isnan(t[:, 2].float()).all()), f"{name}: slices 0 and 2 untouched {tag}")
                    check(bool((act[:, 0] == -7).all()) and bool((act[:, 2] == -7).all()), f"act: slices 0 and 2 untouched {tag}")
                    check(bool(torch.isnan(hh[G * N:].float()).all()) and bool(torch.isnan(cc[G * N:].float()).all()), f"sentinel tail of h and c {tag}")
                    check(not same(hv, h_before), f"the state moved {tag}")
            check(not q11 or not same(vin_ref[1:], _vin_own(raw, grp, n_cops, R)), f"first_agent_state changes the critic rows of agents past the first R={R}")
        env.check_errors()
        env.close()
        print("kernel ok:", roster, R, N, flush=True)


def _vin_own(raw, grp, n_cops, R):
    from as_cops_and_thieves_amd import _learn_native as ln
    N = raw["obs_distance"].shape[0]
    pin = torch.zeros(grp.G, N, 2 * R, dtype=torch.bfloat16, device="cuda")
    vin = torch.zeros(grp.G, N, 4 * R, dtype=torch.bfloat16, device="cuda")
    ln.rollout_pack(raw, grp.indices, n_cops, False, 1.0, 1.0, pin, vin)
    torch.cuda.synchronize()
    return vin[1:]


# ---------------------------------------------------------------------------------------------- 2, 3. a rollout against a from_trainer actor on a twin env
ROSTER, N_ENVS, RAYS, MSC, T, BPTT = (2, 1), 64, 64, 12, 32, 16


def trainer_of(env, fused=True, graph=False, seed=4, **kw):
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, TrainerConfig
    tcfg = TrainerConfig(horizon=T, bptt=BPTT, graph_rollout=graph, graph_update=False, fused_collect=fused, **kw)
    return MAPPOTrainer(env, {"cop": rc(learning_rate=1e-2), "thief": rc(learning_rate=1e-2)}, tcfg, seed=seed)


def replay_on_twin(runner, twin, seed, p_state, starts, tag):
    """Play the rollout the trainer just stored again, with a fused actor over the trainer's own parameters on ``twin``, from ``seed``, the
    recurrent state ``p_state`` and the start flags ``starts``: everything the rollout kept must be bit-equal, tick for tick."""
    from as_cops_and_thieves_amd.selfplay.actor import PolicyActor
    (key, rl), = runner.roles.items()
    b = rl.buf
    actor = PolicyActor.from_trainer(runner, fused=True)
    check(actor.fused, f"{tag}: the actor is fused")
    actor.set_state({key: p_state})
    starts = starts.clone()
    lp = torch.zeros(rl.G, runner.N, device="cuda")
    pin = torch.zeros(rl.G, runner.N, 2 * RAYS, dtype=torch.bfloat16, device="cuda")
    vin = torch.zeros(rl.G, runner.N, 4 * RAYS, dtype=torch.bfloat16, device="cuda")
    real_env = runner.env
    torch.manual_seed(seed)
    bad = set()
    for t in range(T):
        if t % BPTT == 0:
            h, c = actor.state[key]
            if not (same(h, rl.p0w[0][t // BPTT]) and same(c, rl.p0w[1][t // BPTT])):
                bad.add(f"window-start state p0w[{t // BPTT}]")
        runner.env = twin
        runner._pack_native(rl, pin, vin)
        runner.env = real_env
        if not same(pin, b["pin"][:, t]):
            bad.add("pin")
        if not same(vin, b["vin"][:, t]):
            bad.add("vin")
        acts = actor.act(twin, starts, logp_out=lp)
        if not torch.equal(acts.t().long()[rl.indices], b["act"][:, t]):
            bad.add("actions")
        if not same(lp, b["logp"][:, t]):
            bad.add("logp")
        raw = twin.step_raw(acts)
        if not same(raw["reward"].t()[rl.indices], b["rew"][:, t]):
            bad.add("rewards")
        torch.ne(raw["terminated"], 0, out=starts)
        if not torch.equal(starts, runner._done_buf[t]):
            bad.add("done flags")
    torch.cuda.synchronize()
    for what in ("window-start state p0w[0]", "window-start state p0w[1]", "pin", "vin", "actions", "logp", "rewards", "done flags"):
        check(what not in bad, f"{tag}: {what} bit-equal on all {T} ticks")
    check(bool(runner._done_buf.any()) and not bool(runner._done_buf.all()), f"{tag}: episodes end inside the rollout")
    check(len({int(v) for v in b["act"].unique()}) == 4, f"{tag}: all four actions occur")
    h, c = actor.state[key]
    check(same(h, rl.p_state[0]) and same(c, rl.p_state[1]), f"{tag}: the recurrent state after the rollout")


def snapshot(runner, env):
    torch.cuda.synchronize()
    (rl,) = runner.roles.values()
    return twin_of(env, ROSTER, N_ENVS, RAYS, MSC), tuple(s.clone() for s in rl.p_state), runner._starts.clone()


def step_rollout():
    env = env_of(ROSTER, N_ENVS, RAYS, MSC)
    runner = trainer_of(env)
    check(list(runner.roles) == ["cop+thief"], "the roles are stacked in one learner")
    twin, p_state, starts = snapshot(runner, env)
    torch.manual_seed(21)
    runner.collect()
    replay_on_twin(runner, twin, 21, p_state, starts, "eager rollout")
    env.check_errors()


def step_graph():
    env = env_of(ROSTER, N_ENVS, RAYS, MSC)
    runner = trainer_of(env, graph=True)
    (rl,) = runner.roles.values()
    runner.collect()                                             # eager
    check(runner._graph is None, "the first rollout runs eagerly")
    runner.collect()                                             # captured, replayed once
    check(runner._graph is not None, "the second rollout is captured")
    graph = runner._graph
    before = rl.fp.lp.clone()
    runner.update()
    torch.cuda.synchronize()
    check(not same(before, rl.fp.lp), "the update moved the bf16 compute copy")
    twin, p_state, starts = snapshot(runner, env)
    torch.manual_seed(33)
    runner.collect()                                             # replayed
    check(runner._graph is graph, "the third rollout replays the captured graph: no recapture")
    replay_on_twin(runner, twin, 33, p_state, starts, "replayed rollout after an update")
    env.check_errors()                                           # the device error word is 0
    twin.check_errors()


# ---------------------------------------------------------------------------------------------- 4. stored against recomputed log-probabilities
def logp_gap(fused: bool) -> float:
    """The largest |stored logp - the training forward's logp| over the first minibatch of the first update, before any optimiser step."""
    env = env_of(ROSTER, N_ENVS, RAYS, MSC)
    runner = trainer_of(env, fused=fused)
    (rl,) = runner.roles.values()
    figure = []

    def probe(use_graph):
        if figure:
            return
        b, idx = rl.tb, rl.idx
        keep = (~rl.start.index_select(1, idx)).to(torch.float32)
        st = lambda s: s.index_select(2, idx)
        logits, _ = rl.policy.forward(b["pin"], (st(rl.p0[0]), st(rl.p0[1])), keep, select=idx)
        logp = torch.log_softmax(logits.float(), dim=-1).gather(-1, b["act"].index_select(2, idx).unsqueeze(-1)).squeeze(-1)
        figure.append(float((logp - b["logp"].index_select(2, idx)).abs().max()))

    rl.minibatch_step = probe
    torch.manual_seed(5)
    with torch.no_grad():
        runner.collect()
        runner.update()
    env.check_errors()
    env.close()
    return figure[0]


def step_ratio():
    chain = logp_gap(False)
    fused = logp_gap(True)
    print(f"ratio: max |stored logp - training forward's logp|, first minibatch: chain {chain:.6e}  fused {fused:.6e}  "
          f"fused / chain {fused / chain if chain else float('inf'):.3f}", flush=True)
    check(fused <= 2.0 * chain, f"fused {fused:.4e} <= 2 x chain {chain:.4e}")


# ---------------------------------------------------------------------------------------------- 5. end to end
def step_end_to_end():
    import math
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, TrainerConfig
    N = 64
    env = env_of(ROSTER, N, RAYS, 40, track_episodes=True)
    tcfg = TrainerConfig(horizon=16, bptt=16, timesteps=64, policy_freeze_duration=16, opponent_freeze_duration=16, fused_collect=True, frame_skip=2,
                         episode_stats=True, graph_update=False)
    runner = MAPPOTrainer(env, {r: rc(random_timesteps=16, learning_starts=16) for r in ("cop", "thief")}, tcfg, seed=6)
    ticks, updates = [], []
    tick, upd = runner._collect_tick, runner.update
    runner._collect_tick = lambda *a: (ticks.append(1), tick(*a))[1]
    runner.update = lambda *a, **k: (updates.append(len(ticks)), upd(*a, **k))[1]
    stats = runner.train()
    torch.cuda.synchronize()
    print("end to end:", {k: v for k, v in stats.items() if not isinstance(v, list)}, "collect ticks", len(ticks), "updates at", updates, flush=True)
    # rollout 1 is the random phase (today's path), 2 runs eagerly, 3 is captured (its ticks are traced once), 4 is a replay
    check(updates == [0, 16, 32, 32] and runner._graph is not None, "three updates follow fused rollouts: one eager, one captured, one replayed")
    check(all(math.isfinite(v) for k, v in stats.items() if isinstance(v, float)), "the stats are finite")
    check(N * 64 <= stats["env_ticks"] <= 2 * N * 64, f"env_ticks {stats['env_ticks']} counts 1..2 ticks per decision")
    check(stats["episodes"] > 0, "episodes were tracked")
    env.check_errors()
    env.close()
    # one role-training phase: the cops learn through the fused tick, the thieves are a league actor's
    env = env_of(ROSTER, N, RAYS, 40, track_episodes=True)
    tcfg = TrainerConfig(horizon=16, bptt=16, policy_freeze_duration=0, opponent_freeze_duration=0, fused_collect=True, episode_stats=True, graph_update=False)
    runner = MAPPOTrainer(env, {"cop": rc(), "thief": rc()}, tcfg, seed=4, split_roles=True)
    actor = LeagueActor.from_env(env, 2, agents=["thief_0"], fused=True, seed=9)
    actor.set_matchups([(0, 31, {"thief_0": 0}), (31, N, {"thief_0": 1})])
    runner.set_opponent("thief", actor)
    thief_before = runner.roles["thief"].fp.master.clone()
    ticks.clear()
    tick = runner._collect_tick
    runner._collect_tick = lambda *a: (ticks.append(a[0]), tick(*a))[1]
    for _ in range(3):
        runner.collect()
        runner.update()
    stats = runner.read_stats()
    torch.cuda.synchronize()
    check(set(ticks) == {"cop"} and len(ticks) == 32, "the cops' ticks are fused (one eager rollout, one traced for the capture), the thieves' never")
    check(runner._graph is not None, "the role-training rollout is captured")
    check(all(math.isfinite(v) for k, v in stats.items() if isinstance(v, float)) and "cop_0/kl" in stats and "thief_0/kl" not in stats, "role phase: finite stats")
    check(float(runner.roles["cop"].steps.max()) == 6.0 and torch.equal(thief_before, runner.roles["thief"].fp.master), "role phase: the cops alone were updated")
    check(stats["env_ticks"] == N * 48, f"role phase: env_ticks {stats['env_ticks']}")
    env.check_errors()
    env.close()


STEPS = {"kernel": step_kernel, "rollout": step_rollout, "graph": step_graph, "ratio": step_ratio, "end_to_end": step_end_to_end}

if __name__ == "__main__":
    STEPS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("FAILED CHECKS:" if FAILED else "ALL CHECKS PASSED", *FAILED, sep="\n  ", flush=True)
    sys.exit(1 if FAILED else 0)
