"""Frame skip above the env core: ``VecCopsEnv.step(repeat=)`` / ``frame_skip=``, the episode tracker fed windows, the trainer's rollout
with ``TrainerConfig.frame_skip`` (eager and captured) and ``evaluate_league(frame_skip=)``.  The reference of every case is the one-tick
path (a twin env stepped tick by tick, held slots put back as in tests/test_gpu_step_repeat.py) or the tracker's CPU form."""
import numpy as np
import pytest

from tests.test_gpu_step_repeat import _expected

pytestmark = pytest.mark.gpu


def _env(n=70, msc=6, seed=7, **kw):
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    return VecCopsEnv(load_preset("labyrinth", 2, 1), n, num_rays=64, max_step_count=msc, seed=seed, **kw)


def _stagger(*envs, period=6):
    import torch
    for e in envs:
        e.set_env_state(step_count=(torch.arange(e.num_envs, dtype=torch.int32) % period).to(e.device))


def _acts(rng, env):
    import torch
    return torch.from_numpy(rng.integers(0, 4, size=(env.num_envs, 3), dtype=np.int32)).to(env.device)


def test_step_with_repeat_returns_the_dictionaries_over_the_same_buffers():
    import torch
    a, b, c = _env(), _env(frame_skip=3), _env()
    for e in (a, b, c):
        e.reset()
    _stagger(a, b, c)
    rng = np.random.default_rng(0)
    raw = a.raw_outputs()
    cut = False
    for d in range(3):
        acts = _acts(rng, a)
        obs, rew, terms, truncs, infos = a.step(acts, repeat=3)
        obs_b, rew_b, terms_b, _, infos_b = b.step(acts)                       # the constructor's default
        out_c = c.step_raw(acts, repeat=3)
        torch.cuda.synchronize()
        for i, aid in enumerate(a.possible_agents):                             # views of the buffers the kernel wrote, not copies
            assert obs[aid]["distance"].data_ptr() == raw["obs_distance"][:, i].data_ptr()
            assert obs[aid]["object_type"].data_ptr() == raw["obs_type"][:, i].data_ptr()
            assert rew[aid].data_ptr() == raw["reward"][:, i].data_ptr()
            assert torch.equal(obs[aid]["distance"], obs_b[aid]["distance"]) and torch.equal(rew[aid], rew_b[aid])
            assert torch.equal(rew[aid], out_c["reward"][:, i])
        assert out_c is c.raw_outputs() and torch.equal(out_c["ticks"], infos["ticks"])
        assert infos["ticks"].dtype == torch.int32 and bool(((infos["ticks"] >= 1) & (infos["ticks"] <= 3)).all())
        assert torch.equal(infos["ticks"], infos_b["ticks"]) and torch.equal(infos["winner"], infos_b["winner"])
        assert torch.equal(terms["cop_0"], terms_b["cop_0"]) and torch.equal(terms["cop_0"], raw["terminated"].bool())
        assert torch.equal(truncs["thief_0"], raw["truncated"].bool())
        cut |= bool((infos["ticks"] < 3).any())
    assert cut                                                                  # six-tick episodes: some window was cut short
    for k, v in a.get_env_state().items():
        assert torch.equal(v, b.get_env_state()[k]) and torch.equal(v, c.get_env_state()[k]), k
    _, _, _, _, infos1 = a.step(_acts(rng, a))
    assert "ticks" not in infos1 and "ticks" not in a.step(_acts(rng, a), repeat=1)[4]
    for e in (a, b, c):
        e.check_errors()
        e.close()


def test_tracked_env_with_repeat_counts_episodes_in_env_ticks():
    """``episode_stats()`` of a tracked env stepped with repeat = 4 against (1) the tracker's CPU form fed the twin's ticks one by one,
    held slots left out: every integer figure equal; (2) the CPU form fed the same window rows and ``ticks``: the returns bit for bit."""
    import torch
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    N, K = 70, 4
    a, b = _env(N, track_episodes=True), _env(N)
    a.reset(); b.reset()
    _stagger(a, b)
    by_tick, by_window = (EpisodeTracker(N, a.possible_agents, 6) for _ in range(2))
    rng = np.random.default_rng(11)
    t = torch.from_numpy
    for d in range(8):
        acts = _acts(rng, a)
        a.step_raw(acts, repeat=K)
        rows = []
        want, state, jstar, ended = _expected(b._sim, acts, K, rows_out=rows)
        b.set_env_state(**{k: t(np.ascontiguousarray(v)) for k, v in state.items()})
        torch.cuda.synchronize()
        got = {k: a.raw_outputs()[k].cpu().numpy() for k in ("reward", "terminated", "truncated", "winner", "ticks")}
        for k, v in got.items():
            assert np.array_equal(v.view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (d, k)
        by_window.update(t(want["reward"]), t(want["terminated"]), t(want["truncated"]), t(want["winner"]), ticks=t(want["ticks"]))
        for j, r in enumerate(rows):
            live = jstar >= j
            keep = {k: by_tick.state[k].numpy().copy() for k in ("ret_run", "len_run")}
            by_tick.update(t(r["reward"]), t(r["terminated"] * live.astype(np.uint8)), t(r["truncated"]), t(r["winner"]))
            for k, v in keep.items():                                           # a held slot plays no tick
                by_tick.state[k].numpy()[~live] = v[~live]
    stats, tick, window = a.episode_stats(), by_tick.summary(), by_window.summary()
    for key in ("episodes", "cop_wins", "thief_wins", "timeouts", "min_length", "max_length", "mean_length", "length_hist"):
        assert stats[key] == tick[key] == window[key], (key, stats[key], tick[key], window[key])
    assert stats["episodes"] >= N and stats["timeouts"] >= 1 and stats["max_length"] == 6
    for agent in a.possible_agents:
        assert stats[f"mean_return/{agent}"] == window[f"mean_return/{agent}"] and stats[f"std_return/{agent}"] == window[f"std_return/{agent}"]
    a.check_errors(); b.check_errors()
    a.close(); b.close()


def test_trainer_rollout_with_frame_skip_eager_and_captured():
    """Two ``collect()`` calls of a trainer with graphs (the first runs eagerly, the second is captured and replayed) against a trainer
    without, from the same seeds; ``env_ticks`` against the device sum of the env's ``ticks`` after every decision."""
    import torch
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    rc = RoleConfig(random_timesteps=0, learning_starts=0)
    runs = {}
    for graph in (False, True):
        env = _env(32, msc=5, seed=3)       # five-tick episodes: windows of 2, 2 and 1 ticks
        total = torch.zeros((), dtype=torch.int64, device=env.device)
        calls = []
        step_raw = env.step_raw

        def spy(actions, repeat=None, step_raw=step_raw, total=total, calls=calls):
            out = step_raw(actions, repeat=repeat)
            total.add_(out["ticks"].sum())
            calls.append(repeat)
            return out
        env.step_raw = spy
        tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, TrainerConfig(frame_skip=2, horizon=4, graph_rollout=graph, graph_update=False), seed=4)
        torch.manual_seed(77)
        seen = []
        for _ in range(2):
            tr.collect()
            torch.cuda.synchronize()
            (rl,) = tr.roles.values()
            seen.append({k: rl.buf[k].clone() for k in ("rew", "act", "logp")} | {"done": tr._done_buf.clone()})
        assert set(calls) == {2} and tr.timestep == 8
        if graph:
            assert tr._graph is not None and len(calls) == 8          # eager rollout + the capture; the replay calls no Python
        assert tr.read_stats()["env_ticks"] == int(total)              # (captured with the rollout, the spy's sum is replayed with it)
        runs[graph] = (seen, tr.read_stats()["env_ticks"], int(total))
        env.check_errors()
        env.close()
    (eager, ticks_e, total_e), (captured, ticks_g, _) = runs[False], runs[True]
    for i in range(2):
        for k in eager[i]:
            assert torch.equal(eager[i][k], captured[i][k]), (i, k)
    assert ticks_e == total_e == ticks_g and 32 * 8 <= ticks_e < 32 * 8 * 2 and bool(eager[1]["done"].any())


def test_league_lengths_are_env_ticks(tmp_path):
    import torch
    from as_cops_and_thieves_amd.selfplay.stacked import agent_state_dict
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor, PolicyActor
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_league
    N, MSC = 12, 9
    env = _env(N, msc=MSC, seed=5)
    src = PolicyActor.from_checkpoint(None, env, fused=True, seed=1)                # fresh seeded weights, no training
    (grp,) = src.groups.values()
    torch.save({a: {"policy": agent_state_dict(grp.fp, g)["policy"]} for g, a in enumerate(grp.agents)}, tmp_path / "set.pt")
    league = LeagueActor.from_env(env, 3, fused=True)
    for i, agent in enumerate(env.possible_agents):
        league.load_set(i, tmp_path / "set.pt", agent)
    league.set_matchups([(0, 6, {"cop_0": 0, "cop_1": 1, "thief_0": 2}), (6, 12, {"cop_0": 0, "cop_1": 1, "thief_0": 2})])
    torch.manual_seed(9)
    res = evaluate_league(env, league, frame_skip=2)
    env.check_errors()
    length = res["length"].cpu()
    assert res["episodes"] == [6, 6] and bool(((length >= 1) & (length <= MSC)).all())
    assert bool((length == MSC).any()) and res["ticks"] == (MSC + 1) // 2       # nine ticks take five decisions: lengths are not decisions
    # the same slots under a plain fused actor with the league's three sets, stepped with repeat = 2
    env2 = _env(N, msc=MSC, seed=5)
    plain = PolicyActor.from_checkpoint({"cop": tmp_path / "set.pt", "thief": tmp_path / "set.pt"}, env2, fused=True)
    torch.manual_seed(9)
    obs, _ = env2.reset()
    plain.reset()
    starts = torch.ones(N, dtype=torch.bool, device=env2.device)
    open_, played, want = starts.clone(), torch.zeros(N, dtype=torch.int32, device=env2.device), torch.zeros(N, dtype=torch.int32, device=env2.device)
    for _ in range(res["ticks"]):
        actions = plain.act(env2, starts, obs=obs)
        obs, _, terms, _, infos = env2.step(actions, repeat=2)
        played = played + infos["ticks"]
        done = terms["cop_0"]
        want = torch.where(open_ & done, played, want)
        open_, starts = open_ & ~done, done.clone()
    assert torch.equal(want.cpu(), length)
    env.close(); env2.close()
