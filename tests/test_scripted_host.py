"""CPU: the scripted chase / evade opponents -- the torch form against answers derived by hand (tests/scripted_cases.py),
``cat_rollout_scripted_args`` in include/cat_rollout.h against the library and its ctypes mirror, the entry's argument checks (no device
needed), ``LeagueActor.set_matchups`` with the new names, and ``ScriptedActor`` / a mixed league / ``set_opponent`` on the oracle-backed
stand-in env."""
import ctypes as C
import math
import re
import warnings
from pathlib import Path

import pytest
import torch

from as_cops_and_thieves_amd import _learn_native as ln
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
from as_cops_and_thieves_amd.selfplay.scripted import SCRIPTS, ScriptedActor, ScriptedParams, scripted_step
from as_cops_and_thieves_amd.selfplay.self_play import BASELINE_SEGMENTS, evaluate_against_scripts, evaluate_league
from tests import scripted_cases as sc
from tests.fake_env import OracleVecEnv

warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")
ROOT = Path(__file__).resolve().parents[1]
CMAP = load_preset("squarinth", 2, 1).compile()
AGENTS = ["cop_0", "cop_1", "thief_0"]
RC = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=4, learning_starts=8, kl_threshold=0.0)
TC = TrainerConfig(horizon=4, timesteps=16, policy_freeze_duration=8, opponent_freeze_duration=8)


# ---------------------------------------------------------------------------------------------- 1. the rule
def test_the_cones_are_what_the_rule_says():
    for R, sizes in ((8, [1, 1, 1, 1]), (64, [8, 8, 8, 8]), (90, [11, 12, 11, 12])):
        r = torch.arange(R)
        o = ((16 * r + R) % (16 * R)) // (2 * R)
        assert [int((o == 2 * k).sum()) for k in range(4)] == sizes
    for R in range(8, 1025):                                     # never empty, and centred on k pi / 2: the cone holds the ray nearest to it
        o = [((16 * r + R) % (16 * R)) // (2 * R) for r in range(R)]
        for k in range(4):
            assert o[round(k * R / 4) % R] == 2 * k, (R, k)


@pytest.mark.parametrize("c", sc.HAND_CASES, ids=lambda c: c["name"])
def test_torch_form_gives_the_hand_derived_answers(c):
    d, t, u, state, keep = sc.case_tensors(c)
    before = state.clone()
    action, new = scripted_step(d, t, u, state, keep, c["script"], c["target"], c["params"])
    assert int(action) == c["action"] and tuple(new.tolist()) == c["new_state"], (c["name"], int(action), new.tolist())
    assert torch.equal(state, before) and action.dtype == new.dtype == torch.int32        # nothing in place


def test_torch_form_batches_rows_and_leaves_unscripted_rows_alone():
    cases = [c for c in sc.HAND_CASES if c["params"] == sc.DEFAULT]
    cols = list(zip(*[sc.case_tensors(c) for c in cases]))
    d, t, u, state = (torch.stack(x) for x in cols[:4])
    keep = torch.tensor([1.0 if c["keep"] is None else float(c["keep"]) for c in cases])
    script = torch.tensor([c["script"] for c in cases])
    target = torch.tensor([c["target"] for c in cases])
    action, new = scripted_step(d, t, u, state, keep, script, target)
    assert action.tolist() == [c["action"] for c in cases] and new.tolist() == [list(c["new_state"]) for c in cases]
    off = script.clone()
    off[::2] = -1
    action2, new2 = scripted_step(d, t, u, state, keep, off, target)
    assert torch.equal(action2[1::2], action[1::2]) and torch.equal(new2[1::2], new[1::2])
    assert bool((action2[::2] == -1).all()) and torch.equal(new2[::2], state[::2])
    with pytest.raises(ValueError):
        scripted_step(d[:, :7], t[:, :7], u, state, keep, script, target)
    for bad in ({"memory_ticks": -1}, {"clear_min": float("nan")}, {"clear_min": -1.0}, {"turn_prob": 1.5}, {"turn_prob": float("nan")}):
        with pytest.raises(ValueError):
            ScriptedParams(**bad)


# ---------------------------------------------------------------------------------------------- 2. header, library, mirror
def test_scripted_header_matches_the_library_and_the_ctypes_mirror():
    from tests.test_abi_and_isolation import test_learner_kernel_headers_match_the_library_and_the_ctypes_mirror as header_check
    header_check("cat_rollout.h", "cat_rollout_", "ROLLOUT_SYMBOLS", {"cat_rollout_pack_args": "PackArgs", "cat_rollout_sample_args": "SampleArgs",
                                                                     "cat_rollout_post_args": "PostArgs", "cat_rollout_scripted_args": "ScriptedArgs"})
    assert ln.ROLLOUT_SYMBOLS[-1] == "cat_rollout_scripted" == list(ln.MODULES["cat_rollout"][1])[-1] and hasattr(ln.lib(), "cat_rollout_scripted")
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_rollout.h").read_text(), flags=re.S)
    assert int(re.search(r"#define CAT_ROLLOUT_ABI_VERSION (\d+)", code).group(1)) == 1 == ln.lib().cat_rollout_abi_version()
    assert int(re.search(r"#define CAT_ROLLOUT_MAX_SEGMENTS (\d+)", code).group(1)) == ln.SCRIPTED_MAX_SEGMENTS == ln.ACT_MAX_SEGMENTS
    assert (int(re.search(r"#define CAT_ROLLOUT_MIN_RAYS (\d+)", code).group(1)), int(re.search(r"#define CAT_ROLLOUT_MAX_RAYS (\d+)", code).group(1))) == (8, 1024)
    assert re.search(r"CAT_ROLLOUT_CHASE = 0, CAT_ROLLOUT_EVADE = 1", code) and SCRIPTS == {"chase": ln.SCRIPT_CHASE, "evade": ln.SCRIPT_EVADE}
    # N A R G, agent[8], target[8], three parameters, S, seg_start[33], seg_script[8][32] = 1252 bytes -> 1256, then six pointers
    A = ln.ScriptedArgs
    assert (A.agent.offset, A.target.offset, A.memory_ticks.offset, A.clear_min.offset, A.turn_prob.offset, A.S.offset) == (16, 48, 80, 84, 88, 92)
    assert (A.seg_start.offset, A.seg_script.offset, A.obs_distance.offset, A.actions.offset) == (96, 228, 1256, 1296)
    assert C.sizeof(A) == 1304 < 4096


def _args(N=10, A=3, R=64, G=3, S=2, start=(0, 4, 10)):
    a = ln.ScriptedArgs()
    a.N, a.A, a.R, a.G, a.S = N, A, R, G, S
    for g in range(8):
        a.agent[g], a.target[g] = g % 3, 2 if g % 3 < 2 else 1
    a.memory_ticks, a.clear_min, a.turn_prob = 30, 12.0, 0.02
    for s, v in enumerate(start):
        a.seg_start[s] = v
    return a


def test_scripted_entry_rejects_bad_arguments_before_touching_a_device():
    L = ln.lib()
    seen = set()

    def rejected(a, word):
        rc, msg = L.cat_rollout_scripted(C.byref(a), None), L.cat_rollout_last_error()
        assert rc == -1 and word in msg and msg.startswith(b"cat_rollout_scripted: "), (rc, msg, word)
        seen.add(msg)

    assert L.cat_rollout_scripted(None, None) == -1
    rejected(_args(), b"NULL")                                   # a well-formed block reaches the buffer checks (every pointer is NULL)
    for R in (7, 0, 1025):
        rejected(_args(R=R), b"R outside")
    for G in (9, 0):
        rejected(_args(G=G), b"G outside")
    for kw in ({"N": 0}, {"A": 0}, {"A": 9}):
        rejected(_args(**kw), b"dimensions")
    a = _args()
    a.agent[1] = 3                                               # >= A
    rejected(a, b"agent index")
    for script in (2, -2, 7):
        a = _args()
        a.seg_script[2][1] = script
        rejected(a, b"script outside")
    a = _args()
    a.seg_script[1][0], a.seg_script[5][1] = -1, 9               # -1 is "not scripted"; rows of policies beyond G are not read
    rejected(a, b"NULL")
    for target in (0, 3, 4):
        a = _args()
        a.target[1] = target
        rejected(a, b"target")
    rejected(_args(S=0), b"S outside")
    rejected(_args(S=33), b"S outside")
    rejected(_args(start=(1, 4, 10)), b"begin at 0")
    rejected(_args(start=(0, 4, 9)), b"end at N")
    rejected(_args(start=(0, 0, 10)), b"strictly increasing")
    rejected(_args(S=3, start=(0, 6, 4, 10)), b"strictly increasing")
    for v in (float("nan"), -1.0):
        a = _args()
        a.clear_min = v
        rejected(a, b"clear_min")
    for v in (1.5, -0.1, float("nan")):
        a = _args()
        a.turn_prob = v
        rejected(a, b"turn_prob")
    a = _args()
    a.memory_ticks = -1
    rejected(a, b"memory_ticks")
    buf = (C.c_int32 * 64)()
    for missing in ("obs_distance", "obs_type", "uniform", "state", "actions"):
        a = _args()
        for f in ("obs_distance", "obs_type", "uniform", "state", "actions"):
            setattr(a, f, None if f == missing else C.addressof(buf) // 16 * 16 + 16)
        rejected(a, b"NULL")
    a = _args()
    for f in ("obs_distance", "obs_type", "uniform", "state", "actions"):
        setattr(a, f, C.addressof(buf) // 16 * 16 + (20 if f == "state" else 16))
    rejected(a, b"aligned")
    assert len(seen) == 15                                       # each kind of mistake has its own message
    # the older entries keep theirs
    assert L.cat_rollout_sample(C.byref(ln.SampleArgs()), None) == -1 and L.cat_rollout_last_error().startswith(b"cat_rollout_sample: bad dimensions")


def test_scripted_table_applies_the_entrys_rules_in_python():
    t = ln.scripted_table(10, 3, [0, 4, 10], [[0, -1], [1, 1], [-1, 0]])
    assert (t.S, list(t.seg_start[:3]), [list(r[:2]) for r in t.seg_script[:3]]) == (2, [0, 4, 10], [[0, -1], [1, 1], [-1, 0]])
    for start, rows in (([0, 10], [[0], [0]]), ([1, 10], [[0]] * 3), ([0, 9], [[0]] * 3), ([0, 4, 4, 10], [[0] * 3] * 3), ([0, 10], [[2]] * 3),
                        ([0, 10], [[-2]] * 3), ([0], [[]] * 3)):
        with pytest.raises(ValueError):
            ln.scripted_table(10, 3, start, rows)
    with pytest.raises(ValueError):
        ln.scripted_table(33, 3, list(range(34)), [[0] * 33] * 3)


# ---------------------------------------------------------------------------------------------- 3. set_matchups
def test_set_matchups_takes_the_script_names_and_still_rejects_others():
    env = OracleVecEnv(CMAP, 7, num_rays=16, max_step_count=12, seed=3)
    actor = LeagueActor.from_env(env, 3, fused=False)
    ok = {"cop_0": 0, "cop_1": 1, "thief_0": 2}
    actor.set_matchups([(0, 7, ok)])
    assert actor.script_table is None and actor.script_state is None          # nothing scripted: nothing allocated
    actor.set_matchups([(0, 3, dict(ok, thief_0="evade")), (3, 5, {"cop_0": "chase", "cop_1": "random", "thief_0": 2}), (5, 7, ok)])
    assert actor.table.table == [[0, -1, 0], [1, -1, 1], [-1, 2, 2]]           # the league kernel is told "random" for a scripted agent
    assert actor.script_table.rows == [[-1, 0, -1], [-1, -1, -1], [1, -1, -1]] and actor.script_table.start == actor.table.start == [0, 3, 5, 7]
    assert actor.script_state.shape == (3, 7, 4) and actor.script_state.dtype == torch.int32
    for word in ("greedy", "Chase", "flee", "", None, 1.0, True):
        with pytest.raises(ValueError):
            actor.set_matchups([(0, 7, dict(ok, thief_0=word))])
    assert actor.segments == [(0, 3), (3, 5), (5, 7)]                        # a refused table leaves the current one in place
    actor.set_matchups([(0, 7, ok)])
    assert actor.script_table is None


# ---------------------------------------------------------------------------------------------- 4. on the stand-in env
def test_scripted_actor_plays_the_torch_form_on_the_stand_in_env():
    env = OracleVecEnv(CMAP, 6, num_rays=16, max_step_count=40, seed=3)
    actor = ScriptedActor(env, {"cop_0": "chase", "cop_1": "chase"})
    assert (actor.agents, actor.env_agents, actor.N, actor.R, actor.fused) == (["cop_0", "cop_1"], AGENTS, 6, 16, False)
    assert actor.actions.shape == (6, 3) and actor.segments == [(0, 6)] and actor.table.rows == [[0], [0]] and actor.targets == [2, 2]
    obs, _ = env.reset()
    starts = torch.ones(6, dtype=torch.bool)
    state = torch.zeros(2, 6, 4, dtype=torch.int32)
    actions = torch.full((6, 3), 9, dtype=torch.int32)
    torch.manual_seed(4)
    gen_state = torch.random.get_rng_state()
    for tick in range(30):
        got = actor.act(env, starts, obs=obs, actions=actions)
        assert got is actions and bool((actions[:, 2] == 9).all())           # the thief's column is not the actor's
        after = torch.random.get_rng_state()
        torch.random.set_rng_state(gen_state)
        u = torch.rand(2, 6)                                                 # one draw of [G, N] per tick
        assert torch.equal(torch.random.get_rng_state(), after)
        d = torch.stack([obs[a]["distance"] for a in ("cop_0", "cop_1")])
        t = torch.stack([obs[a]["object_type"] for a in ("cop_0", "cop_1")])
        want, state = scripted_step(d, t, u, state, (~starts).view(1, 6), 0, torch.tensor([[2], [2]]))
        assert torch.equal(actions[:, :2], want.t()) and torch.equal(actor.state, state), tick
        actions[:, 2] = 9
        step = actions.clone()
        step[:, 2] = tick % 4
        obs, _, terms, _, _ = env.step(step)
        starts = terms["cop_0"].clone()
        gen_state = after
    assert bool((actor.state[..., 0] == 1).all()) and len(set(actions[:, :2].flatten().tolist())) > 1
    saved = actor.get_state()
    actor.reset(torch.tensor([True, False, False, False, False, True]))
    assert bool((actor.state[:, [0, 5]] == 0).all()) and torch.equal(actor.state[:, 1:5], saved[:, 1:5])
    actor.set_state(saved)
    assert torch.equal(actor.state, saved)
    table = actor.table
    actor.set_segments([(0, 2, {"cop_0": "chase", "cop_1": None}), (2, 6, {"cop_0": None, "cop_1": "evade"})])
    assert actor.table is not table and actor.segments == [(0, 2), (2, 6)]   # a new object: a trainer recaptures
    before = actor.state.clone()
    actions.fill_(9)
    actor.act(env, obs=obs, actions=actions)
    assert bool((actions[2:, 0] == 9).all()) and bool((actions[:2, 1] == 9).all()) and bool((actions[:2, 0] != 9).all()) and bool((actions[2:, 1] != 9).all())
    assert torch.equal(actor.state[0, 2:], before[0, 2:]) and torch.equal(actor.state[1, :2], before[1, :2])
    for bad in ({"thief_7": "evade"}, {"cop_0": "flee"}, {}):
        with pytest.raises(ValueError):
            ScriptedActor(env, bad)
    with pytest.raises(ValueError):
        actor.set_segments([(0, 5, {"cop_0": "chase", "cop_1": None})])


def test_league_with_mixed_segments_plays_scripts_beside_networks_on_the_stand_in_env():
    segments = [(0, 2, {"cop_0": 0, "cop_1": 1, "thief_0": "evade"}), (2, 5, {"cop_0": "chase", "cop_1": "random", "thief_0": 2}),
                (5, 7, {"cop_0": 0, "cop_1": 1, "thief_0": 2})]
    plain = [(lo, hi, {a: "random" if v in SCRIPTS else v for a, v in who.items()}) for lo, hi, who in segments]
    runs = {}
    for name, table in (("mixed", segments), ("plain", plain)):
        env = OracleVecEnv(CMAP, 7, num_rays=16, max_step_count=12, seed=3)
        actor = LeagueActor.from_env(env, 3, fused=False, seed=4)
        actor.set_matchups(table)
        obs, _ = env.reset()
        starts = torch.ones(7, dtype=torch.bool)
        actor.reset()
        torch.manual_seed(9)
        runs[name] = (actor, actor.act(env, starts, greedy=True, obs=obs).clone(), obs)
    (actor, mixed, obs), (other, base, _) = runs["mixed"], runs["plain"]
    (key,) = actor.state
    # the network-played cells do not depend on who else is scripted (greedy: no draw of theirs), state included
    for lo, hi, who in segments:
        for g, a in enumerate(AGENTS):
            if isinstance(who[a], int):
                assert torch.equal(mixed[lo:hi, g], base[lo:hi, g]), (lo, a)
                assert all(torch.equal(x[:, g, lo:hi], y[:, g, lo:hi]) for x, y in zip(actor.state[key], other.state[key])), (lo, a)
    # the scripted cells are the rule on their rows, from the draws after the segment's others
    torch.manual_seed(9)
    u = torch.rand(2)                                            # segment 0: no "random" agent, then thief_0's rows
    want, st = scripted_step(obs["thief_0"]["distance"][0:2], obs["thief_0"]["object_type"][0:2], u, torch.zeros(2, 4, dtype=torch.int32), None, 1, 1)
    assert torch.equal(mixed[0:2, 2], want) and torch.equal(actor.script_state[2, 0:2], st)
    torch.randint(0, 4, (3, 3))                                  # segment 1: cop_1's "random" draw over [G, rows], then cop_0's rows
    u = torch.rand(3)
    want, st = scripted_step(obs["cop_0"]["distance"][2:5], obs["cop_0"]["object_type"][2:5], u, torch.zeros(3, 4, dtype=torch.int32), None, 0, 2)
    assert torch.equal(mixed[2:5, 0], want) and torch.equal(actor.script_state[0, 2:5], st)
    assert bool((actor.script_state[1] == 0).all()) and bool((actor.script_state[2, 2:] == 0).all()) and bool((actor.script_state[0, 5:] == 0).all())
    h, _ = actor.state[key]
    assert bool((h[:, 2, 0:2] == 0).all()) and bool((h[:, 0, 2:5] == 0).all())          # a scripted agent's recurrent rows are left alone
    saved = actor.get_state()
    assert torch.equal(saved["scripted"], actor.script_state) and bool((saved["scripted"] != 0).any())
    actor.reset()
    assert bool((actor.script_state == 0).all())
    actor.set_state(saved)
    assert torch.equal(actor.script_state, saved["scripted"]) and "scripted" not in other.get_state()


def test_evaluate_against_scripts_plays_four_segments_in_one_pass():
    env = OracleVecEnv(CMAP, 8, num_rays=16, max_step_count=12, seed=5)
    runner = MAPPOTrainer(OracleVecEnv(CMAP, 4, num_rays=16, max_step_count=12, seed=1), {"cop": RC, "thief": RC}, TC, seed=7)
    torch.manual_seed(3)
    res = evaluate_against_scripts(env, runner, 2, fused=False)
    assert res["segments"] == list(BASELINE_SEGMENTS) and res["episodes"] == [2, 2, 2, 2] and 1 <= res["ticks"] <= 12
    assert [c + t + o for c, t, o in zip(res["cop_wins"], res["thief_wins"], res["timeouts"])] == [2] * 4
    assert all(1 <= v <= 12 for v in res["mean_length"]) and res["cop_win_rate"] == [c / 2 for c in res["cop_wins"]]
    with pytest.raises(ValueError):
        evaluate_against_scripts(env, runner, 3, fused=False)
    # a ScriptedActor over every agent is an actor evaluate_league takes as it is
    actor = ScriptedActor(env, {"cop_0": "chase", "cop_1": "chase", "thief_0": "evade"})
    out = evaluate_league(env, actor)
    assert out["episodes"] == [8] and out["cop_wins"][0] + out["thief_wins"][0] + out["timeouts"][0] == 8


# ---------------------------------------------------------------------------------------------- 5. as a training opponent
def test_set_opponent_with_a_scripted_actor_trains_the_other_role_eagerly():
    env = OracleVecEnv(CMAP, 4, num_rays=16, max_step_count=12, seed=1)
    runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=7, split_roles=True)
    thief_key, cop_key = "thief", "cop"
    actor = ScriptedActor(env, {"thief_0": "evade"})
    runner.set_opponent(thief_key, actor)
    assert list(runner.learners) == [cop_key] and runner._opponent_tables() == (actor.table,) and not runner._opponents_capturable()
    frozen = runner.roles[thief_key].fp.master.clone()
    before = runner.roles[cop_key].fp.master.clone()
    runner.reset_episodes()
    runner.train(16)
    assert torch.equal(runner.roles[thief_key].fp.master, frozen) and not torch.equal(runner.roles[cop_key].fp.master, before)
    assert bool((actor.state[..., 0] == 1).all())                # the actor played every slot
    assert all(math.isfinite(v) for k, v in runner.read_stats().items() if k.endswith("_loss"))
    with pytest.raises(ValueError):
        runner.set_opponent(cop_key, ScriptedActor(env, {"thief_0": "evade"}))


# ---------------------------------------------------------------------------------------------- 6. the users
def test_self_play_with_baseline_eval_writes_baselines_json(tmp_path):
    import json
    from as_cops_and_thieves_amd.selfplay.self_play import TrainingConfig, run_self_play
    factory = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=12, seed=s)
    lines = []
    run_self_play("squarinth", 8, tmp_path / "on", iterations=2, training=TrainingConfig(n_trial_episodes=3, num_opponents_to_evaluate=2),
                  trainer_cfg=TC, role_cfg={"cop": RC, "thief": RC}, env_factory=factory, seed=0, baseline_eval=True, baseline_episodes=2,
                  log=lambda *a: lines.append(" ".join(map(str, a))))
    book = json.loads((tmp_path / "on" / "baselines.json").read_text())
    assert [b["iteration"] for b in book] == [0, 1] and sum("baselines, cop win rate" in line for line in lines) == 2
    for b in book:
        assert b["segments"] == list(BASELINE_SEGMENTS) and b["episodes"] == [2] * 4
        assert [c + t + o for c, t, o in zip(b["cop_wins"], b["thief_wins"], b["timeouts"])] == [2] * 4
    run_self_play("squarinth", 8, tmp_path / "off", iterations=1, training=TrainingConfig(n_trial_episodes=3, num_opponents_to_evaluate=2),
                  trainer_cfg=TC, role_cfg={"cop": RC, "thief": RC}, env_factory=factory, seed=0, log=lambda *a: None)
    assert not (tmp_path / "off" / "baselines.json").exists()                # off by default
    with pytest.raises(ValueError):
        run_self_play("squarinth", 8, tmp_path / "bad", iterations=1, env_factory=factory, baseline_eval=True, role_training=True, log=lambda *a: None)


def test_crossplay_scripted_adds_a_chase_row_and_an_evade_column(tmp_path):
    from as_cops_and_thieves_amd.selfplay.actor import PolicyActor
    from as_cops_and_thieves_amd.selfplay.crossplay import crossplay
    from as_cops_and_thieves_amd.selfplay.stacked import agent_state_dict
    factory = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=12, seed=s)
    env = factory(2, 0)
    for role, d, seeds in (("cop", "cops", (0, 1)), ("thief", "thieves", (2,))):
        (tmp_path / d).mkdir()
        for it, seed in enumerate(seeds):
            (grp,) = PolicyActor.from_checkpoint(None, env, fused=False, seed=seed).groups.values()
            torch.save({a: {"policy": agent_state_dict(grp.fp, g)["policy"]} for g, a in enumerate(grp.agents)}, tmp_path / d / f"{role}_iter_{it}.pt")
    table = crossplay(tmp_path / "cops", tmp_path / "thieves", "squarinth", 2, random_column=True, scripted=True, fused=False, env_factory=factory, seed=4)
    assert table["cops"] == ["cop_iter_0.pt", "cop_iter_1.pt", "chase"] and table["thieves"] == ["thief_iter_0.pt", "random", "evade"]
    for k in ("cop_win_rate", "cop_wins", "thief_wins", "timeouts", "mean_length"):
        assert len(table[k]) == 3 and all(len(row) == 3 for row in table[k]), k
    assert all(table["cop_wins"][i][j] + table["thief_wins"][i][j] + table["timeouts"][i][j] == 2 for i in range(3) for j in range(3))
    plain = crossplay(tmp_path / "cops", tmp_path / "thieves", "squarinth", 2, random_column=True, fused=False, env_factory=factory, seed=4)
    assert plain["cops"] == table["cops"][:2] and plain["thieves"] == table["thieves"][:2]         # off by default


def test_watch_parses_its_script_option():
    from as_cops_and_thieves_amd.selfplay import watch
    with pytest.raises(SystemExit):
        watch.main(["--out", "nowhere", "--script", "cop=flee"])
    with pytest.raises(SystemExit):
        watch.main(["--out", "nowhere", "--script", "robber=chase"])
