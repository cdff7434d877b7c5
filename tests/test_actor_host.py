"""CPU: the inference-only ``PolicyActor`` on the oracle-backed stand-in env -- its unfused path against today's evaluation loops bit for
bit, checkpoint loading (policy blocks only, both layouts, per-role sources), greedy and random action selection -- and include/cat_act.h
against the library and its ctypes mirror."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.selfplay.actor import PolicyActor, first_max_index
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
from as_cops_and_thieves_amd.selfplay.self_play import (TrainingConfig, evaluate_agent, evaluate_agents, evaluate_agents_tracked, mean_reward_per_tick,
                                                        run_self_play)
from as_cops_and_thieves_amd.selfplay.stacked import _net_shapes
from tests.fake_env import OracleVecEnv
from tests.test_episodes_host import TrackedOracleVecEnv, sim_state_bytes

ROOT = Path(__file__).resolve().parents[1]
CMAP = load_preset("squarinth", 2, 1).compile()
RC = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=4, learning_starts=8, kl_threshold=0.0)
TC = TrainerConfig(horizon=4, timesteps=16, policy_freeze_duration=8, opponent_freeze_duration=8)
# 400-tick episodes: captures and timeouts fall on different ticks from slot to slot (tests/test_episodes_host.py)
PLAIN_LONG = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=400, seed=s)
TRACKED_LONG = lambda n, s: TrackedOracleVecEnv(CMAP, n, num_rays=16, max_step_count=400, seed=s)


@pytest.mark.parametrize("factory,fn,kw", [(PLAIN_LONG, evaluate_agents, {}), (TRACKED_LONG, evaluate_agents_tracked, {"poll_every": 5})])
def test_unfused_actor_equals_todays_evaluation_bit_for_bit(factory, fn, kw):
    """Three evaluations in a row on one env from the same generator state and env seed, with and without the actor: the same pairs,
    and the generator and the env left in the same state after each."""
    runs = []
    for with_actor in (False, True):
        env = factory(24, 5)
        assert env.possible_agents == ["cop_0", "cop_1", "thief_0"]
        runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=2)
        actor = PolicyActor.from_trainer(runner, fused=False) if with_actor else None
        torch.manual_seed(1234)
        seen = []
        for _ in range(3):
            res = fn(env, runner, 24, actor=actor, **kw) if with_actor else fn(env, runner, 24, **kw)
            seen.append((res, torch.get_rng_state().numpy().tobytes(), sim_state_bytes(env)))
        runs.append(seen)
    for k, ((res_a, rng_a, st_a), (res_b, rng_b, st_b)) in enumerate(zip(*runs)):
        assert res_a == res_b, (k, res_a, res_b)
        assert rng_a == rng_b, k
        assert st_a == st_b, k
    assert all(res[0] > 0 and res[1] > 0 for res, _, _ in runs[1]), [r for r, _, _ in runs[1]]      # captures and timeouts both occur
    assert len({res for res, _, _ in runs[1]}) > 1
    assert not actor.fused and actor.state_bytes == 2 * 3 * 24 * 128 * 4


def test_actor_with_random_roles_equals_todays_evaluation():
    out = []
    for with_actor in (False, True):
        env = OracleVecEnv(CMAP, 6, num_rays=16, max_step_count=12, seed=9)
        runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=4)
        torch.manual_seed(99)
        kw = {"actor": PolicyActor.from_trainer(runner, fused=False)} if with_actor else {}
        out.append((evaluate_agents(env, runner, 5, random_roles=("thief",), **kw), torch.get_rng_state().numpy().tobytes()))
    assert out[0] == out[1]


def test_mean_reward_per_tick_through_an_actor_equals_the_trainers():
    out = []
    for with_actor in (False, True):
        env = OracleVecEnv(CMAP, 6, num_rays=16, max_step_count=12, seed=9)
        runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=4)
        torch.manual_seed(7)
        kw = {"actor": PolicyActor.from_trainer(runner, fused=False)} if with_actor else {}
        out.append((mean_reward_per_tick(env, runner, 20, random_roles=("cop",), **kw), torch.get_rng_state().numpy().tobytes()))
    assert out[0] == out[1] and set(out[0][0]) == {"cop_0", "cop_1", "thief_0"}


def test_evaluate_agent_through_an_actor_books_what_the_trainer_books(tmp_path):
    """``evaluate_agent``'s own loading -- the learned role from the trainer, each opponent from its archive file -- into an actor and
    into a second trainer: equal policy parameters afterwards, the same outcomes booked, the same log lines."""
    import random
    from as_cops_and_thieves_amd.selfplay import archive
    env = OracleVecEnv(CMAP, 8, num_rays=16, max_step_count=400, seed=1)
    learned, old_a, old_b = (MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=s) for s in (21, 22, 23))
    tc = TrainingConfig(n_trial_episodes=8, num_opponents_to_evaluate=2)
    seen = {}
    for mode in ("trainer", "actor"):
        arch = tmp_path / mode / "thieves"
        arch.mkdir(parents=True)
        for it, old in enumerate((old_a, old_b)):
            ck = tmp_path / mode / f"joint_iter_{it}_full_agent.pt"
            torch.save(old.state_dict(), ck)
            archive.add_policy_to_archive(str(ck), arch, it, "thief")
        eval_env = OracleVecEnv(CMAP, 8, num_rays=16, max_step_count=400, seed=77)
        if mode == "actor":
            evaluator = PolicyActor.from_checkpoint(None, eval_env, fused=False, seed=5)
            eval_env.reset()                                 # a trainer resets its env once when it is built: the same env state either way
        else:
            evaluator = MAPPOTrainer(eval_env, {"cop": RC, "thief": RC}, TC, seed=5)
        lines = []
        torch.manual_seed(3)
        res = evaluate_agent(eval_env, evaluator, learned, "cop", "thief", arch, tc, random.Random(0), log=lines.append, fused_eval=mode == "actor")
        fp = next(iter((evaluator.groups if mode == "actor" else evaluator.roles).values())).fp
        seen[mode] = (res, lines, {n: fp.views[n].detach().clone() for n in fp.names if n.startswith("policy.")})
    assert seen["trainer"][0] == seen["actor"][0] and len(seen["actor"][0]) == 2
    assert seen["trainer"][1] == seen["actor"][1]
    assert all(torch.equal(v, seen["actor"][2][n]) for n, v in seen["trainer"][2].items())
    rl, g = learned.learner_of("cop_1")
    assert torch.equal(seen["actor"][2]["policy.lstm.weight_hh_l0"][1], rl.fp.views["policy.lstm.weight_hh_l0"][g].detach())   # the learned cops


def test_self_play_with_fused_eval_runs_and_archives(tmp_path):
    import json
    lines = []
    res = run_self_play("squarinth", 8, tmp_path / "run", fused_eval=True, training=TrainingConfig(n_trial_episodes=6, num_opponents_to_evaluate=2),
                        trainer_cfg=TC, eval_envs=8, role_cfg={"cop": RC, "thief": RC}, env_factory=TRACKED_LONG, iterations=3, tracked_eval=True,
                        log=lambda *a: lines.append(" ".join(map(str, a))))
    assert len(res["iterations"]) == 3 and [len(h["evaluations"]["cop"]) for h in res["iterations"]] == [0, 1, 2]
    for d in ("cops", "thieves"):
        rates = json.loads((tmp_path / "run" / d / "win_rates.json").read_text())
        assert len(rates) >= 1, d
    assert sum(" vs " in line for line in lines) == 6 and (tmp_path / "run" / "joint_iter_2_full_agent.pt").exists()


def _policy_bytes(R, G, itemsize):
    return G * itemsize * sum(int(np.prod(s)) for s in _net_shapes("policy", R).values())


@pytest.mark.parametrize("layout", ["cat", "reference"])
def test_checkpoint_round_trip_loads_the_policy_blocks_only(tmp_path, layout):
    env = OracleVecEnv(CMAP, 4, num_rays=16, max_step_count=12, seed=1)
    runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=7)
    sd = runner.state_dict()
    if layout == "reference":                                # what skrl's MAPPO.save writes: no trainer position
        del sd[MAPPOTrainer.META_KEY]
    torch.save(sd, tmp_path / "ck.pt")
    actor = PolicyActor.from_checkpoint(tmp_path / "ck.pt", env, fused=False, seed=99)
    (grp,) = actor.groups.values()
    assert all(n.startswith("policy.") for n in grp.fp.names) and not hasattr(grp.fp, "grad")
    for g, a in enumerate(grp.agents):
        rl, gr = runner.learner_of(a)
        for n in grp.fp.names:
            assert torch.equal(grp.fp.views[n][g], rl.fp.views[n][gr].detach()), (a, n)
    assert actor.parameter_bytes == _policy_bytes(16, 3, 4) == PolicyActor.from_trainer(runner, fused=False).parameter_bytes
    assert grp.fp.lp.numel() * 4 < actor.parameter_bytes + 3 * 64 * 4          # nothing but the blocks and their alignment padding
    with pytest.raises(ValueError):
        PolicyActor.from_checkpoint(tmp_path / "ck.pt", env, fused=True)       # no GPU here: a loud error, not a fall-back
    # the loaded actor plays what the trainer's own policies play
    torch.manual_seed(5)
    a = evaluate_agents(env, runner, 4)
    torch.manual_seed(5)
    b = evaluate_agents(OracleVecEnv(CMAP, 4, num_rays=16, max_step_count=12, seed=1), None, 4, actor=actor)
    assert a == b


def test_cop_and_thief_from_different_files(tmp_path):
    env = OracleVecEnv(CMAP, 4, num_rays=16, max_step_count=12, seed=1)
    one, two = (MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=s) for s in (11, 12))
    torch.save(one.state_dict(), tmp_path / "one.pt")
    torch.save(two.state_dict(), tmp_path / "two.pt")
    actor = PolicyActor.from_checkpoint({"cop": tmp_path / "one.pt", "thief": tmp_path / "two.pt"}, env, fused=False)
    (grp,) = actor.groups.values()
    name = "policy.policy_head.0.weight"
    for g, a in enumerate(grp.agents):
        src, other = (one, two) if a.startswith("cop") else (two, one)
        rl, gr = src.learner_of(a)
        assert torch.equal(grp.fp.views[name][g], rl.fp.views[name][gr].detach())
        rl, gr = other.learner_of(a)
        assert not torch.equal(grp.fp.views[name][g], rl.fp.views[name][gr].detach())
    before = grp.fp.views[name].clone()
    actor.load(tmp_path / "two.pt", roles=["cop"])           # as evaluate_agent swaps one role's opponent in
    assert torch.equal(grp.fp.views[name][2], before[2]) and not torch.equal(grp.fp.views[name][0], before[0])
    with pytest.raises(KeyError):
        actor.load({"cop_0": {}}, roles=["thief"])


def _chain_logits(runner, env, obs):
    from as_cops_and_thieves_amd import packing
    (rl,) = runner.roles.values()
    pin = torch.stack([packing.pack_policy_input(obs[a]) for a in rl.agents])
    with torch.no_grad():
        logits, _ = rl.policy.forward(pin.unsqueeze(1), rl.policy.initial_state(env.num_envs), None)
    return logits[:, 0].float()


def test_greedy_is_the_first_maximal_index_and_random_roles_are_uniform():
    N = 64
    env = OracleVecEnv(CMAP, N, num_rays=16, max_step_count=12, seed=3)
    runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=5)
    obs, _ = env.reset()
    z = _chain_logits(runner, env, obs)
    want = torch.stack([torch.tensor([min(j for j in range(4) if row[j] == max(row)) for row in zg.tolist()]) for zg in z])
    actor = PolicyActor.from_trainer(runner, fused=False)
    got = actor.act(env, greedy=True, obs=obs).clone()
    assert torch.equal(got.long(), want.t())
    assert torch.equal(first_max_index(torch.tensor([[1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 4.0]])), torch.tensor([1, 0, 3]))
    # random thieves: uniform over the four actions, and the cops' (network) rows do not move
    actor.reset()
    counts = torch.zeros(4)
    for _ in range(60):
        actor.reset()
        acts = actor.act(env, greedy=True, random_roles=("thief",), obs=obs)
        assert torch.equal(acts[:, :2].long(), want.t()[:, :2])
        counts += torch.bincount(acts[:, 2].long(), minlength=4).float()
    freq = counts / counts.sum()
    assert float((freq - 0.25).abs().max()) < 0.04, freq      # 3840 draws: the standard deviation of a frequency is 0.007
    assert actor.actions.data_ptr() == acts.data_ptr()        # a persistent buffer


def test_reset_zeroes_the_masked_slots_and_state_copies_round_trip():
    env = OracleVecEnv(CMAP, 5, num_rays=16, max_step_count=12, seed=3)
    actor = PolicyActor.from_checkpoint(None, env, fused=False, seed=1)
    actor.act(env)
    (st,) = actor.state.values()
    assert all(bool((t != 0).any(dim=-1).all()) for t in st)
    kept = actor.get_state()
    actor.reset(torch.tensor([True, False, False, True, False]))
    for t in st:
        assert not bool(t[:, :, [0, 3]].any()) and bool((t[:, :, [1, 2, 4]] != 0).any(dim=-1).all())
    actor.set_state(kept)
    assert all(torch.equal(a, b) for a, b in zip(actor.state[next(iter(actor.state))], kept[next(iter(kept))]))
    actor.reset()
    assert not any(bool(t.any()) for t in st)


def test_act_header_matches_the_library_and_the_ctypes_mirror():
    """The checks tests/test_abi_and_isolation.py applies to the other learner headers, on include/cat_act.h."""
    from tests.test_abi_and_isolation import test_learner_kernel_headers_match_the_library_and_the_ctypes_mirror as header_check
    from tests.test_abi_and_isolation import test_product_package_never_references_the_oracle as isolation_check
    header_check("cat_act.h", "cat_act_", "ACT_SYMBOLS", {"cat_act_dims": "ActDims", "cat_act_params": "ActParams", "cat_act_args": "ActArgs"})
    isolation_check()
    from as_cops_and_thieves_amd import _learn_native as ln
    assert ln.SOURCES[-1].name == "cat_act.hip" and ln.HEADERS[-1].name == "cat_act.h"


def test_ctypes_struct_sizes_equal_the_headers_layout():
    from as_cops_and_thieves_amd import _learn_native as ln
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_act.h").read_text(), flags=re.S)
    assert int(re.search(r"#define CAT_ACT_MAX_AGENTS (\d+)", code).group(1)) == ln.ACT_MAX_AGENTS == 8
    # cat_act_dims: 4 x int32; cat_act_params: 16 pointers + int64; cat_act_args: dims, agent[8], mode / random_mask / row_tile, two
    # floats, pad (72 bytes, 8-aligned), two pointers, params, seven pointers
    assert C.sizeof(ln.ActDims) == 16 and C.sizeof(ln.ActParams) == 16 * 8 + 8
    assert C.sizeof(ln.ActArgs) == 16 + 8 * 4 + 3 * 4 + 2 * 4 + 4 + 2 * 8 + C.sizeof(ln.ActParams) + 7 * 8
    assert ln.ActArgs.obs_distance.offset == 72 and ln.ActArgs.p.offset == 88 and ln.ActArgs.h.offset == 88 + 136
    L = ln.lib()
    assert L.cat_act_supported(C.byref(ln.ActDims(3, 4096, 3, 64))) == 1 and L.cat_act_supported(C.byref(ln.ActDims(5, 1, 5, 90))) == 1
    for bad in ((3, 10, 3, 72), (9, 10, 3, 64), (0, 10, 3, 64), (3, 0, 3, 64), (3, 10, 9, 64)):
        assert L.cat_act_supported(C.byref(ln.ActDims(*bad))) == 0
        a = ln.ActArgs()
        a.d = ln.ActDims(*bad)
        assert L.cat_act_step(C.byref(a), None) == -1 and b"dimensions" in L.cat_act_last_error()      # BAD_ARG before any device call
    a = ln.ActArgs()
    a.d = ln.ActDims(3, 10, 3, 64)
    assert L.cat_act_step(C.byref(a), None) == -1 and b"NULL" in L.cat_act_last_error()
