"""Episode accounting on the GPU (include/cat_episodes.h): the two kernels against the CPU form of ``EpisodeTracker`` bit for bit on
the env core's own outputs, cross-checks against the env's state that need no restatement, ``VecCopsEnv(track_episodes=True)``
through its three entries, and the trainer with the rollout graph."""
import numpy as np
import pytest

from tests.util import compiled, free_positions

pytestmark = pytest.mark.gpu

FIVE = ["agh-map", "grandbyrinth", "labyrinth", "lbirinth", "squarinth"]
STREAMS = ("reward", "terminated", "truncated", "winner")
SLOT_FIELDS = ("ret_run", "len_run", "finished", "cop_wins", "thief_wins", "timeouts", "len_sum", "len_min", "len_max", "ret_sum", "ret_sq",
               "len_hist")
AGENTS = ["cop_0", "cop_1", "thief_0"]


def record(names, N, T, max_steps, seed=77):
    """T ticks of the env core under its synthetic actions, all four streams kept: device tensors [T, N, ...]."""
    import torch
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim
    maps = [compiled(n, 2, 1) for n in names]
    slot = (np.arange(N) % len(maps)).astype(np.int32) if len(maps) > 1 else None
    sim = CatSim(SimConfig(n_envs=N, n_cops=2, n_thieves=1, n_rays=64, max_step_count=max_steps, seed=seed), maps, slot, device="cuda:0")
    sim.reset()
    rows = sim.rollout_fused(T, None, tick=3, auto_reset=True)
    torch.cuda.synchronize()
    rows = {k: rows[k].clone() for k in STREAMS}
    assert sim.device_errors() == 0
    sim.close()
    return rows


def state_bytes(tracker):
    import torch
    torch.cuda.synchronize()
    st = tracker.per_slot()
    return {k: st[k].cpu().numpy().tobytes() for k in SLOT_FIELDS}


def quota_of(N):
    import torch
    return (torch.arange(N, dtype=torch.int32) * 7) % 5        # 0 .. 4 episodes, differently from slot to slot


# ---------------------------------------------------------------------------------------------- 6. kernel == CPU tracker
@pytest.mark.parametrize("quota", [False, True])
@pytest.mark.parametrize("names,N,T", [(["squarinth"], 1, 61), (["squarinth"], 63, 61), (["squarinth"], 200, 45), (FIVE, 1000, 61),
                                       (["squarinth"], 4096, 64), (FIVE, 4096, 37)])
def test_kernels_equal_the_cpu_tracker_bit_for_bit(names, N, T, quota):
    import torch
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    max_steps = 9
    rows = record(names, N, T, max_steps)
    host_rows = [rows[k].cpu() for k in STREAMS]
    assert int(host_rows[1].sum(0).min()) >= T // max_steps >= 4         # every slot ends several episodes
    whole, single, host = (EpisodeTracker(N, AGENTS, max_steps, d) for d in ("cuda:0", "cuda:0", "cpu"))
    if quota:
        for tr in (whole, single, host):
            tr.set_quota(quota_of(N))
    whole.update(*(rows[k] for k in STREAMS))
    for t in range(T):
        single.update(*(rows[k][t] for k in STREAMS))
    host.update(*host_rows)
    want = {k: host.per_slot()[k].numpy().tobytes() for k in SLOT_FIELDS}
    for name, tr in (("one launch", whole), ("tick by tick", single)):
        got = state_bytes(tr)
        for k in SLOT_FIELDS:
            assert got[k] == want[k], (name, k)
        assert tr.summary_block() == host.summary_block(), name
        assert tr.summary() == host.summary(), name
    s = whole.summary()
    assert s["episodes"] == (int(torch.minimum(host_rows[1].sum(0).to(torch.int32), quota_of(N)).sum()) if quota else int(host_rows[1].sum()))
    assert s["episodes"] > 0 or N == 1
    # clear() and abandon() are the same on both devices
    mask = torch.arange(N) % 3 == 0
    for tr in (whole, host):
        tr.clear()
        tr.abandon(mask.to(tr.device))
        tr.update(*((rows[k] if tr is whole else rows[k].cpu()) for k in STREAMS))
    got, want = state_bytes(whole), {k: host.per_slot()[k].numpy().tobytes() for k in SLOT_FIELDS}
    assert all(got[k] == want[k] for k in SLOT_FIELDS) and whole.summary() == host.summary()


# ---------------------------------------------------------------------------------------------- 10. reproducible
def test_two_runs_give_byte_identical_summary_blocks():
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    blocks, tails = [], []
    for _ in range(2):
        rows = record(["squarinth"], 4096, 64, 9)
        tr = EpisodeTracker(4096, AGENTS, 9, "cuda:0")
        tr.update(*(rows[k] for k in STREAMS))
        blocks.append(tr.summary_block())
        tails.append(tr._tail.cpu().numpy().tobytes())         # the summary block and the histogram as the kernels left them
    assert blocks[0] == blocks[1] and tails[0] == tails[1] and blocks[0]["episodes"] > 4096 * 6


# ---------------------------------------------------------------------------------------------- 7. cross-checks
def test_cross_checks_against_the_env_state_with_captures_and_timeouts():
    """Tracking starts at a reset whose injected positions put a thief inside the capture radius of cop 0 in most slots: the first
    episodes end in captures, the ones after the auto-reset (random spawns, 15-tick cap) mostly in timeouts.

    "Every counted timeout has length max_step_count" is checked per call through what the per-slot state shows of it without a log of
    the single episodes -- necessary conditions, a bound and not the property itself: a slot with a timeout has len_max == max_step_count
    and len_sum >= timeouts * max_step_count, with equality where every counted episode of the slot was a timeout, and the histogram bin
    of that length holds at least the timeouts.  The property itself follows from the last assertion: the figures equal those of the CPU
    tracker fed by the CPU env core, which ``tests/test_episodes_host.py`` holds against a per-episode loop."""
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    from as_cops_and_thieves_amd.maps import load_preset
    from oracle.cat_oracle import OracleSim
    N, max_steps = 64, 15
    env = VecCopsEnv(load_preset("squarinth"), N, num_rays=64, max_step_count=max_steps, seed=4, track_episodes=True)
    cpu = OracleSim(env._cfg, env._compiled)
    positions = free_positions(cpu, env._compiled[0], np.random.default_rng(3), spread=12.0)
    # the CPU side first: the same positions and the same synthetic actions give captures AND timeouts
    total = 10 + 25 + 5
    want = EpisodeTracker(N, env.possible_agents, max_steps)
    cpu.reset(positions=positions)
    for t in range(total):
        c = cpu.step(cpu.random_actions(t))
        want.update(*(torch.from_numpy(c[k].copy()) for k in STREAMS))
        cpu.reset(mask=c["terminated"].copy())
    w = want.summary()
    assert w["cop_wins"] >= 1 and w["timeouts"] >= 1, w

    def check(ctx):
        st = env.episode_tracker.per_slot()
        torch.cuda.synchronize()
        assert torch.equal(st["len_run"], env.get_env_state()["step_count"]), ctx
        s = env.episode_stats()
        assert s["cop_wins"] + s["thief_wins"] == s["episodes"] and s["timeouts"] <= s["thief_wins"] and sum(s["length_hist"]) == s["episodes"], (ctx, s)
        # every counted timeout has length max_step_count: a slot's longest counted episode, and the histogram bin of that length
        t = st["timeouts"].cpu().numpy()
        assert (st["len_max"].cpu().numpy()[t > 0] == max_steps).all() and (st["len_sum"].cpu().numpy() >= t * max_steps).all(), ctx
        only = t == st["finished"].cpu().numpy()
        assert (st["len_sum"].cpu().numpy()[only] == t[only] * max_steps).all(), ctx
        assert s["length_hist"][(max_steps - 1) * 64 // max_steps] >= s["timeouts"] and s["max_length"] <= max_steps, ctx
        return s

    env.reset(options={"positions": torch.from_numpy(positions)})
    check("after the reset")
    for t in range(10):
        env.step_raw(env.random_actions(t))
        check(f"step_raw {t}")
    env.rollout_random(25, tick0=10)
    check("rollout_random")
    for t in range(35, 40):
        env.step(env.random_actions(t))
        s = check(f"step {t}")
    assert s["cop_wins"] >= 1 and s["timeouts"] >= 1, s
    assert s == w                                          # and, the env core being bit-identical to the CPU one, the same figures
    env.check_errors()
    # a masked reset abandons the masked slots only
    before = env.episode_tracker.per_slot()["len_run"].clone()
    mask = torch.arange(N) % 2 == 0
    env.reset(options={"mask": mask})
    after = env.episode_tracker.per_slot()["len_run"]
    assert int(after[mask.to(after.device)].abs().sum()) == 0 and torch.equal(after[1::2], before[1::2])
    check("masked reset")
    assert env.episode_stats(clear=True)["episodes"] == s["episodes"] and env.episode_stats()["episodes"] == 0
    env.close()


# ---------------------------------------------------------------------------------------------- 8. the env's three entries
def test_step_step_raw_and_rollout_random_account_alike():
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    N, T, tick0 = 200, 53, 500
    make = lambda track: VecCopsEnv(load_preset("squarinth"), N, num_rays=64, max_step_count=9, seed=6, track_episodes=track)
    raw, dic, res, chunked, plain = make(True), make(True), make(True), make(True), make(False)
    chunked.TRACKED_ROLLOUT_BYTES = 7 * N * (4 * 3 + 3)    # 7 ticks per resident launch: several chunks and a ragged last one
    for e in (raw, dic, res, chunked, plain):
        e.reset()
    for t in range(T):
        raw.step_raw(raw.random_actions(tick0 + t))
        dic.step(dic.random_actions(tick0 + t))
    res.rollout_random(T, tick0=tick0)
    chunked.rollout_random(T, tick0=tick0)
    plain.rollout_random(T, tick0=tick0)
    torch.cuda.synchronize()
    want = state_bytes(raw.episode_tracker)
    for name, e in (("step", dic), ("rollout_random", res), ("rollout_random in chunks", chunked)):
        got = state_bytes(e.episode_tracker)
        for k in SLOT_FIELDS:
            assert got[k] == want[k], (name, k)
        assert e.episode_stats() == raw.episode_stats()
    assert raw.episode_stats()["episodes"] >= N * (T // 9)
    assert chunked._tracked_rows["reward"].shape[0] == 7 and res._tracked_rows["reward"].shape[0] == T - 1
    # tracking changes nothing of the env: state and outputs byte-equal to an env without it, driven the same way
    ref_state, ref_out = plain.get_env_state(), plain.raw_outputs()
    for name, e in (("step_raw", raw), ("step", dic), ("rollout_random", res), ("chunked", chunked)):
        st, out = e.get_env_state(), e.raw_outputs()
        for k in ref_state:
            assert st[k].cpu().numpy().tobytes() == ref_state[k].cpu().numpy().tobytes(), (name, k)
        for k in ref_out:
            assert out[k].cpu().numpy().tobytes() == ref_out[k].cpu().numpy().tobytes(), (name, k)
    assert not hasattr(plain, "_tracked_rows")
    with pytest.raises(RuntimeError, match="track_episodes"):
        plain.episode_stats()
    with pytest.raises(RuntimeError, match="track_episodes"):
        plain.episode_tracker
    with pytest.raises(ValueError, match="auto_reset"):
        VecCopsEnv(load_preset("squarinth"), 8, auto_reset=False, track_episodes=True)
    for e in (raw, dic, res, chunked, plain):
        e.check_errors()
        e.close()


# ---------------------------------------------------------------------------------------------- tracked evaluation on the device
def test_tracked_evaluation_equals_evaluate_agents_over_evaluations_in_a_row():
    """Three evaluations in a row on one env each, plain and tracked: same results, and after every one the generators and the env's
    state stand where ``evaluate_agents`` leaves them."""
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_agents, evaluate_agents_tracked
    N, n_episodes = 256, 200
    tcfg = TrainerConfig(horizon=16, graph_rollout=False, graph_update=False)
    runs = []
    for flag in (False, True):
        env = VecCopsEnv(load_preset("squarinth"), N, num_rays=64, max_step_count=300, seed=5, track_episodes=flag)
        runner = MAPPOTrainer(env, {"cop": RoleConfig(), "thief": RoleConfig()}, tcfg, seed=2)
        torch.manual_seed(1234)
        seen = []
        for _ in range(3):
            res = evaluate_agents_tracked(env, runner, n_episodes, poll_every=32) if flag else evaluate_agents(env, runner, n_episodes)
            torch.cuda.synchronize()
            state = {k: v.cpu().numpy().tobytes() for k, v in env.get_env_state().items()}
            seen.append((res, torch.get_rng_state().numpy().tobytes(), torch.cuda.get_rng_state(env.device).numpy().tobytes(), state))
        if flag:
            s = env.episode_stats()
            assert s["episodes"] == n_episodes and s["cop_wins"] >= 1 and s["thief_wins"] >= 1 and s["min_length"] < s["max_length"], s
        env.check_errors()
        env.close()
        runs.append(seen)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a[0] == b[0], (k, a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2], k
        for key in a[3]:
            assert a[3][key] == b[3][key], (k, key)
    assert all(r[0][0] > 0 and r[0][1] > 0 for r in runs[1]), [r[0] for r in runs[1]]


# ---------------------------------------------------------------------------------------------- 9. trainer, graph rollout
def test_trainer_accounts_every_tick_of_eager_and_replayed_rollouts():
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    N, H, k = 256, 16, 5
    rc = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0)
    digests = []
    for flag in (False, True):
        env = VecCopsEnv(load_preset("squarinth"), N, num_rays=64, max_step_count=20, seed=2, track_episodes=flag)
        tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, TrainerConfig(horizon=H, policy_freeze_duration=0, opponent_freeze_duration=0,
                                                                       graph_rollout=True, episode_stats=flag), seed=1)
        for i in range(k):                                 # the first rollout runs eagerly, the second is captured, all later ones replay
            tr.collect()
            tr.update()
            if flag:
                st = env.episode_tracker.per_slot()
                torch.cuda.synchronize()
                assert (st["len_sum"] + st["len_run"]).tolist() == [(i + 1) * H] * N, f"rollout {i}"
                assert torch.equal(st["len_run"], env.get_env_state()["step_count"])
        assert tr._graph is not None
        digests.append(tr.param_digest())
        stats = tr.read_stats()
        assert ("episodes" in stats) == flag
        if flag:
            assert stats["episodes"] >= N * (k * H // 20 - 1) and 0.0 <= stats["cop_win_rate"] <= 1.0 and 1.0 <= stats["mean_episode_length"] <= 20.0
            assert all(f"mean_return/{a}" in stats for a in env.possible_agents)
        env.close()
    assert digests[0] == digests[1]


def test_train_call_with_the_resident_random_phase_accounts_every_tick():
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    N = 64
    rc = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=32, learning_starts=48, kl_threshold=0.0)
    digests = []
    for flag in (False, True):
        env = VecCopsEnv(load_preset("squarinth"), N, num_rays=64, max_step_count=20, seed=5, track_episodes=flag)
        tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, TrainerConfig(horizon=16, timesteps=96, policy_freeze_duration=0, opponent_freeze_duration=0,
                                                                       episode_stats=flag), seed=0)
        stats = tr.train()             # 32 ticks in one resident launch, then an eager rollout, a captured one and two replays
        digests.append(tr.param_digest())
        if flag:
            st = env.episode_tracker.per_slot()
            torch.cuda.synchronize()
            assert (st["len_sum"] + st["len_run"]).tolist() == [96] * N
            assert stats["episodes"] == int(st["finished"].sum()) >= N * 3
        env.close()
    assert digests[0] == digests[1]
