"""Role training (the reference's ``train_role`` / ``_orchestrate_training_phase``) on the CPU stand-in env, unfused: a ``LeagueActor`` over ONE
role's agents, ``MAPPOTrainer.set_opponent`` and the ``run_self_play(role_training=True)`` phases."""
import json
import warnings

import pytest
import torch

from as_cops_and_thieves_amd.episodes import EpisodeTracker
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
from as_cops_and_thieves_amd.selfplay.self_play import TrainingConfig, even_segments, run_self_play, train_role_league
from tests.fake_env import OracleVecEnv

warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")
CMAP = load_preset("squarinth").compile()
RC = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0, kl_threshold=0.0)
TC = TrainerConfig(horizon=4, timesteps=8, policy_freeze_duration=0, opponent_freeze_duration=0)
N = 9
SEGMENTS = [(0, 3), (3, 7), (7, 9)]


class TrackedEnv(OracleVecEnv):
    """The stand-in env with the tracker surface of ``VecCopsEnv(track_episodes=True)``."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.episode_tracker = EpisodeTracker(self.num_envs, self.possible_agents, self.max_step_count)

    def reset(self, seed=None, options=None):
        self.episode_tracker.abandon()
        return super().reset(seed, options)

    def step(self, actions):
        res = super().step(actions)
        rew = torch.stack([res[1][a] for a in self.possible_agents], dim=1)
        self.episode_tracker.update(rew, res[2][self.possible_agents[0]], res[3][self.possible_agents[0]], res[4]["winner"])
        return res

    def episode_stats(self, clear=False, segments=None):
        return self.episode_tracker.summary()


def make_env(n=N, seed=1, cls=OracleVecEnv):
    return cls(CMAP, n, num_rays=16, max_step_count=6, seed=seed)


def thief_actor(env, sets=3, middle=1):
    actor = LeagueActor.from_env(env, sets, agents=["thief_0"], fused=False, seed=11)
    with torch.no_grad():           # freshly initialised policies are all near uniform: sets 1 and 2 get a will of their own (actions 0 and 3)
        for k, liked in ((1, 0), (2, 3)):
            if k < sets:
                actor.bank.views["policy.policy_head.4.bias"][k] = torch.tensor([8.0 if j == liked else -8.0 for j in range(4)])
    actor.set_matchups([(lo, hi, {"thief_0": k}) for (lo, hi), k in zip(SEGMENTS, (0, middle, "random"))])
    return actor


def trainer_with_opponent(env, tcfg=TC, middle=1, seed=0):
    tr = MAPPOTrainer(env, {"cop": RC, "thief": RC}, tcfg, seed=seed, split_roles=True)
    assert list(tr.roles) == ["cop", "thief"]
    tr.set_opponent("thief", thief_actor(env, middle=middle))
    return tr


def test_split_roles_changes_the_stacking_not_the_weights():
    a = MAPPOTrainer(make_env(), {"cop": RC, "thief": RC}, TC, seed=3)
    b = MAPPOTrainer(make_env(), {"cop": RC, "thief": RC}, TC, seed=3, split_roles=True)
    assert list(a.roles) == ["cop+thief"] and list(b.roles) == ["cop", "thief"]
    for ag in a.agents:
        for kind in ("policy", "value"):
            for k, v in a.agent_models(ag)[kind].items():
                assert torch.equal(v, b.agent_models(ag)[kind][k]), (ag, kind, k)


def test_actor_over_one_role_leaves_the_other_columns_alone():
    env = make_env()
    obs, _ = env.reset()
    actor = thief_actor(env)
    assert actor.agents == ["thief_0"] and actor.env_agents == env.possible_agents and actor.group.indices == [2]
    assert actor.state["thief"][0].shape[1] == 1                                  # the state of one agent
    actions = torch.full((N, 3), 7, dtype=torch.int32)
    out = actor.act(env, torch.ones(N, dtype=torch.bool), obs=obs, actions=actions)
    assert out is actions and bool((actions[:, :2] == 7).all()) and bool(((actions[:, 2] >= 0) & (actions[:, 2] < 4)).all())
    assert bool((actor.actions == 0).all())                                       # its own buffer was not written
    own = actor.act(env, obs=obs)                                                 # the default: today's buffer
    assert own is actor.actions and bool((own[:, :2] == 0).all())
    with pytest.raises(ValueError):
        actor.set_matchups([(0, N, {"cop_0": 0, "cop_1": 0, "thief_0": 0})])       # names agents the actor does not cover
    with pytest.raises(ValueError):
        actor.act(env, obs=obs, actions=torch.zeros(N, 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        LeagueActor.from_env(env, 2, agents=["thief_9"], fused=False)


def test_opponent_role_is_played_not_trained():
    env = make_env()
    tr = trainer_with_opponent(env)
    cop, thief = tr.roles["cop"], tr.roles["thief"]
    held = [t.clone() for t in (thief.fp.master, thief.m, thief.v, thief.steps)]
    cop0 = cop.fp.master.clone()
    seen = []
    step = env.step
    env.step = lambda actions: (seen.append(actions.clone()), step(actions))[1]
    stats = tr.train(8)
    assert all(torch.equal(a, b) for a, b in zip(held, (thief.fp.master, thief.m, thief.v, thief.steps)))
    assert not torch.equal(cop0, cop.fp.master) and float(cop.steps.max()) == 4.0    # two updates of one epoch x two minibatches, of the cops alone
    assert all(not bool(v.any()) for v in thief.buf.values())                        # no rollout row of the thieves
    assert bool(cop.buf["pin"].any()) and bool(cop.buf["logp"].any())
    assert len(seen) == 8 and all(bool(((a >= 0) & (a < 4)).all()) for a in seen)
    assert not any(k.startswith("thief_0/") for k in stats) and "cop_0/kl" in stats
    assert set(tr.state_dict()) == {"cop_0", "cop_1", "__cat__"}
    digest = tr.param_digest()
    tr.set_opponent("thief", None)
    assert set(tr.state_dict()) == {"cop_0", "cop_1", "thief_0", "__cat__"} and tr.param_digest() != digest
    assert all(torch.equal(a, b) for a, b in zip(held, (thief.fp.master, thief.m, thief.v, thief.steps)))


def _rollout_buffers(middle):
    torch.manual_seed(123)
    tr = trainer_with_opponent(make_env(), middle=middle)
    torch.manual_seed(5)
    tr.collect()
    tr.collect()
    return {k: v.clone() for k, v in tr.roles["cop"].buf.items() if k in ("pin", "vin", "act", "logp", "rew")}, tr._done_buf.clone()


def test_another_set_in_one_segment_leaves_the_other_slots_alone():
    (a, da), (b, db), (c, dc) = _rollout_buffers(1), _rollout_buffers(1), _rollout_buffers(2)
    lo, hi = SEGMENTS[1]
    outside = [n for n in range(N) if not lo <= n < hi]
    for k in a:
        assert torch.equal(a[k], b[k]), k                                            # the same seeds give the same rollout
        assert torch.equal(a[k][:, :, outside], c[k][:, :, outside]), k
    assert torch.equal(da[:, outside], dc[:, outside])
    assert any(not torch.equal(a[k][:, :, lo:hi], c[k][:, :, lo:hi]) for k in a)     # the segment itself saw another opponent


def test_set_opponent_refuses_what_does_not_fit():
    env = make_env()
    tr = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, split_roles=True)
    with pytest.raises(ValueError):
        tr.set_opponent("cop", thief_actor(env))                                     # an actor over the wrong agents
    with pytest.raises(ValueError):
        tr.set_opponent("thief", LeagueActor.from_env(env, 2, fused=False))          # ... over all agents
    with pytest.raises(ValueError):
        tr.set_opponent("thief", thief_actor(make_env(n=N + 1)))                     # ... over another batch
    with pytest.raises(ValueError):
        tr.set_opponent("robber", None)
    joint = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC)
    with pytest.raises(ValueError):
        joint.set_opponent("thief", thief_actor(env))                                # one stacked learner: no such key
    tr.set_opponent("thief", thief_actor(env))
    cops = LeagueActor.from_env(env, 2, agents=["cop_0", "cop_1"], fused=False)
    cops.set_matchups([(0, N, {"cop_0": 0, "cop_1": 1})])
    with pytest.raises(ValueError):
        tr.set_opponent("cop", cops)                                                 # nobody would be left to learn


def test_read_stats_reports_the_opponent_segments():
    env = make_env(cls=TrackedEnv)
    tr = trainer_with_opponent(env, TrainerConfig(horizon=4, timesteps=16, policy_freeze_duration=0, opponent_freeze_duration=0, episode_stats=True))
    stats = tr.train(16)
    segs = stats["segments"]
    assert segs == env.episode_tracker.segment_summary([0, 3, 7, 9]) and len(segs) == 3
    assert sum(s["episodes"] for s in segs) == stats["episodes"] > 0
    assert all({"episodes", "cop_wins", "thief_wins", "timeouts", "mean_length"} <= set(s) for s in segs)
    tr.set_opponent("thief", None)
    assert "segments" not in tr.read_stats()


def test_frame_skip_runs_through():
    from tests.test_frame_skip_host import _skip_env_class
    env = make_env(cls=_skip_env_class())
    tr = trainer_with_opponent(env, TrainerConfig(horizon=4, timesteps=8, policy_freeze_duration=0, opponent_freeze_duration=0, frame_skip=2))
    stats = tr.train(8)
    assert env.calls == [2] * 8 and N * 8 <= stats["env_ticks"] <= 2 * N * 8          # the opponent decided once per decision


def test_even_segments_and_config_range(tmp_path):
    assert even_segments(96, 3) == [(0, 32), (32, 64), (64, 96)] and even_segments(10, 4) == [(0, 3), (3, 6), (6, 8), (8, 10)]
    assert TrainingConfig().num_training_opponents == 8
    env = make_env()
    tr = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, split_roles=True)
    for bad in (0, 33, 2.0, True):                  # checked where role training reads it: the simultaneous loop never does
        tc = TrainingConfig(num_training_opponents=bad)
        with pytest.raises(ValueError):
            train_role_league(tr, env, make_env(), "cop", "thief", {"cop": tmp_path / "cops", "thief": tmp_path / "thieves"}, tc, None)
        with pytest.raises(ValueError):
            run_self_play("squarinth", 8, tmp_path, iterations=1, training=tc, role_training=True, **KW)


KW = dict(trainer_cfg=TC, role_cfg={"cop": RC, "thief": RC}, log=lambda *a: None,
          env_factory=lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=6, seed=s))


def test_role_training_self_play_books_and_archives_per_phase(tmp_path):
    tc = TrainingConfig(n_trial_episodes=3, num_training_opponents=2, policy_sample_strategy="pfsp")
    res = run_self_play("squarinth", 8, tmp_path, iterations=2, training=tc, role_training=True, **KW)
    wr = lambda d: json.loads((tmp_path / d / "win_rates.json").read_text()) if (tmp_path / d / "win_rates.json").exists() else {}
    games = lambda d: {k: v["games"] for k, v in wr(d).items() if v["games"]}
    (c0, t0), (c1, t1) = (it["phases"] for it in res["iterations"])
    # iteration 0: the cops meet an empty thief archive -- "random", nothing booked; the thieves meet the cops just archived
    assert c0["opponents"] == ["random"] and c0["outcomes"] == {} and c0["segments"] == [(0, 8)]
    assert t0["opponents"] == ["cop_iter_0.pt"] and list(t0["outcomes"]) == ["cop_iter_0.pt"]
    # iteration 1: one archived thief for the cops; two archived cops, on two segments, for the thieves
    assert c1["opponents"] == ["thief_iter_0.pt"] and list(c1["outcomes"]) == ["thief_iter_0.pt"]
    assert sorted(t1["opponents"]) == ["cop_iter_0.pt", "cop_iter_1.pt"] == sorted(t1["outcomes"]) and t1["segments"] == [(0, 4), (4, 8)]
    # one outcome per drawn opponent, in the OPPONENT role's archive
    assert games("thieves") == {"thief_iter_0.pt": 1} and games("cops") == {"cop_iter_0.pt": 2, "cop_iter_1.pt": 1}
    assert all(isinstance(v, bool) for ph in (t0, c1, t1) for v in ph["outcomes"].values())
    # every phase added one entry to its own role's archive only
    for role, d in (("cop", "cops"), ("thief", "thieves")):
        assert sorted(p.name for p in (tmp_path / d).glob("*.pt")) == [f"{role}_iter_{i}.pt" for i in range(2)]
        sd = torch.load(tmp_path / f"{role}_iter_1_full_agent.pt", weights_only=True)
        assert {a.split("_")[0] for a in sd if a != "__cat__"} == {role}
        assert max(float(st["step"]) for a in sd if a != "__cat__" for st in sd[a]["optimizer"]["state"].values()) == 4.0
    assert not list(tmp_path.glob("joint_iter_*")) and not (tmp_path / "role_training.json").exists()
    # a resumed run continues after the highest archived iteration
    res = run_self_play("squarinth", 8, tmp_path, iterations=1, training=tc, role_training=True, **KW)
    assert [h["iteration"] for h in res["iterations"]] == [2] and (tmp_path / "thief_iter_2_full_agent.pt").exists()


def test_role_training_resumes_between_the_phases_of_an_iteration(tmp_path):
    tc = TrainingConfig(n_trial_episodes=2, num_training_opponents=2)
    run_self_play("squarinth", 8, tmp_path, iterations=1, training=tc, role_training=True, **KW)
    (tmp_path / "thieves" / "thief_iter_0.pt").unlink()                              # as if the run had stopped after the cop phase
    res = run_self_play("squarinth", 8, tmp_path, iterations=2, training=tc, role_training=True, **KW)
    assert [(h["iteration"], [ph["role"] for ph in h["phases"]]) for h in res["iterations"]] == [(0, ["thief"]), (1, ["cop", "thief"])]
    for role, d in (("cop", "cops"), ("thief", "thieves")):
        assert sorted(p.name for p in (tmp_path / d).glob("*.pt")) == [f"{role}_iter_{i}.pt" for i in range(2)]
    res = run_self_play("squarinth", 8, tmp_path, iterations=1, training=tc, role_training=True, resume=False, **KW)
    assert [(h["iteration"], len(h["phases"])) for h in res["iterations"]] == [(0, 2)]   # without resume nothing is skipped


def test_role_training_writes_per_opponent_figures(tmp_path):
    tc = TrainingConfig(n_trial_episodes=2, num_training_opponents=2)
    kw = dict(KW, env_factory=lambda n, s: TrackedEnv(CMAP, n, num_rays=16, max_step_count=6, seed=s))
    run_self_play("squarinth", 8, tmp_path, iterations=2, training=tc, role_training=True, episode_stats=True, **kw)
    log = json.loads((tmp_path / "role_training.json").read_text())
    assert [(e["iteration"], e["role"]) for e in log] == [(0, "cop"), (0, "thief"), (1, "cop"), (1, "thief")]
    assert [len(e["segments"]) for e in log] == [1, 1, 1, 2] == [len(e["opponents"]) for e in log]
    assert all(set(s) == {"episodes", "cop_wins", "thief_wins", "timeouts", "mean_length"} for e in log for s in e["segments"])


def test_role_training_off_is_the_call_it_was(tmp_path):
    tc = TrainingConfig(n_trial_episodes=2, num_opponents_to_evaluate=2)
    a = run_self_play("squarinth", 8, tmp_path / "a", iterations=2, training=tc, **KW)
    b = run_self_play("squarinth", 8, tmp_path / "b", iterations=2, training=tc, role_training=False, **KW)
    assert a["param_digest"] == b["param_digest"]
    assert sorted(p.name for p in (tmp_path / "a").rglob("*")) == sorted(p.name for p in (tmp_path / "b").rglob("*"))
    assert (tmp_path / "b" / "joint_iter_1_full_agent.pt").exists() and not (tmp_path / "b" / "role_training.json").exists()


def test_role_training_refuses_what_it_cannot_combine(tmp_path):
    with pytest.raises(ValueError):
        run_self_play("squarinth", 8, tmp_path, iterations=1, role_training=True, tracked_eval=True, **KW)
    with pytest.raises(ValueError):
        run_self_play("squarinth", 8, tmp_path, iterations=1, role_training=True, eval_envs=5, **KW)
    env = make_env()
    joint = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC)
    with pytest.raises(ValueError):
        train_role_league(joint, env, make_env(), "cop", "thief", {"cop": tmp_path / "cops", "thief": tmp_path / "thieves"}, TrainingConfig(), None)
