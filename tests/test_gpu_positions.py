"""GPU: ``cat_render_positions_update`` (include/cat_render.h) against the NumPy form of ``positions.PositionTracker`` -- every count
is an integer, so the comparison is exact -- and the tracker behind ``VecCopsEnv(track_positions=CELL)``: ``step_raw``,
``rollout_random``, frame skip, a captured step, and ``evaluate_league(..., positions=True)``."""
import numpy as np
import pytest

from tests.positions_cases import synthetic_stream

pytestmark = pytest.mark.gpu

SHAPES = [  # T, N, A, n_cops, R, cell, W, H
    (1, 1, 2, 1, 7, 1, 40, 30),
    (61, 63, 3, 2, 64, 8, 100, 60),
    (37, 200, 5, 3, 90, 5, 100, 60),
    (64, 257, 3, 2, 90, 16, 1280, 800),
    (5, 70, 16, 8, 3, 4, 64, 64),
    (33, 65, 3, 2, 64, 4, 1280, 800),          # 320 x 200 = 64000 cells per plane: a grid wider than 2^16 cells with A = 3
]
G = 3
_CACHE = {}


def _case(shape):
    """The stream of a shape and what the CPU form makes of it, with and without obs_type: computed once, never changed."""
    import torch
    from as_cops_and_thieves_amd.positions import PositionTracker
    if shape not in _CACHE:
        T, N, A, n_cops, R, cell, W, H = shape
        pos, term, obs, group, quota = synthetic_stream(20 + len(_CACHE), T, N, A, R, W, H, G)
        want = {}
        for with_obs in (True, False):
            tr = PositionTracker(N, [f"a{i}" for i in range(A)], n_cops, (W, H), cell, G)
            tr.set_groups(group)
            tr.set_quota(quota)
            tr.update(torch.from_numpy(pos), torch.from_numpy(term), torch.from_numpy(obs) if with_obs else None)
            want[with_obs] = tr.counts()
        _CACHE[shape] = (pos, term, obs, group, quota, want)
    return _CACHE[shape]


def _same(tracker, want, ctx):
    got = tracker.counts()
    for k in ("counts", "outside", "rows", "done"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (ctx, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("with_obs", [True, False], ids=["obs_type", "no obs_type"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d N%d A%d nc%d R%d cell%d %dx%d" % s)
def test_kernel_equals_the_cpu_form_byte_for_byte(shape, with_obs):
    import torch
    from as_cops_and_thieves_amd.positions import SEEN, PositionTracker
    T, N, A, n_cops, R, cell, W, H = shape
    pos, term, obs, group, quota, want = _case(shape)
    want = want[with_obs]
    if with_obs and T * N >= 1000:
        assert want["counts"][:, SEEN].sum() > 0 and want["outside"].sum() > 0       # the streams reach every branch
    dev = torch.device("cuda")
    p, t, o = torch.from_numpy(pos).to(dev), torch.from_numpy(term).to(dev), torch.from_numpy(obs).to(dev) if with_obs else None
    at_once, by_row = (PositionTracker(N, [f"a{i}" for i in range(A)], n_cops, (W, H), cell, G, device=dev) for _ in range(2))
    for tr in (at_once, by_row):
        tr.set_groups(group)
        tr.set_quota(quota)
    at_once.update(p, t, o)                                  # one launch of T rows
    for k in range(T):                                       # T launches of one row
        by_row.update(p[k], t[k], None if o is None else o[k])
    _same(at_once, want, "one launch")
    _same(by_row, want, "row by row")


def test_no_group_and_no_quota_pointer_count_every_row():
    """The entry itself with group = quota = NULL, and an obs_type view at an odd byte offset."""
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    from as_cops_and_thieves_amd.positions import PositionTracker
    T, N, A, n_cops, R, cell, W, H = 9, 45, 3, 1, 13, 8, 100, 60
    pos, term, obs, _, _ = synthetic_stream(3, T, N, A, R, W, H, 1)
    cpu = PositionTracker(N, ["a", "b", "c"], n_cops, (W, H), cell)
    cpu.update(torch.from_numpy(pos), torch.from_numpy(term), torch.from_numpy(obs))
    dev = torch.device("cuda")
    gpu = PositionTracker(N, ["a", "b", "c"], n_cops, (W, H), cell, device=dev)
    s = gpu.tensors()
    flat = torch.zeros(obs.size + 1, dtype=torch.uint8, device=dev)
    flat[1:] = torch.from_numpy(obs).to(dev).reshape(-1)
    ln.positions_update(torch.from_numpy(pos).to(dev), torch.from_numpy(term).to(dev), flat[1:].view(T, N, A, R), None, None,
                        s["counts"], s["outside"], s["rows"], s["done"], n_cops, cell)
    _same(gpu, cpu.counts(), "NULL group and quota")
    assert gpu.counts()["rows"][0] == T * N


def _env(N=63, seed=6, **kw):
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    return VecCopsEnv(load_preset("squarinth"), N, num_rays=64, max_step_count=9, seed=seed, **kw)


def _record(env, out):
    return {k: out[k].cpu().clone() for k in ("team_positions", "terminated", "obs_type")}


def test_env_step_raw_and_rollout_random_feed_the_tracker():
    """61 step_raw ticks, then rollout_random(61), against the CPU tracker fed the rows of an untracked twin env played tick by tick.
    Seed 6: on the CPU oracle the 122 ticks hold thousands of seen and of unseen non-terminal rows for either role (asserted below)."""
    import torch
    from as_cops_and_thieves_amd.positions import OCC, SEEN, SPAWN, PositionTracker
    N, cell = 63, 8
    env, small, twin = _env(track_positions=cell), _env(track_positions=cell, position_exposure=False), _env()
    small.TRACKED_ROLLOUT_BYTES = 7 * N * small._tracked_row_bytes(small._tracked_keys())      # several chunks and a ragged last one
    for e in (env, small, twin):
        e.reset()
    rows = []
    for t in range(122):
        rows.append(_record(twin, twin.step_raw(twin.random_actions(t))))
    for t in range(61):
        env.step_raw(env.random_actions(t))
        small.step_raw(small.random_actions(t))
    env.rollout_random(61, tick0=61)
    small.rollout_random(61, tick0=61)
    torch.cuda.synchronize()
    for e in (env, small, twin):
        e.check_errors()
    rec = {k: torch.stack([r[k] for r in rows]) for k in rows[0]}
    window = tuple(int(v) for v in env._compiled[0].window)
    cpu = PositionTracker(N, env.possible_agents, 2, window, cell)
    cpu.update(rec["team_positions"], rec["terminated"], rec["obs_type"])
    want = cpu.counts()
    _same(env.position_tracker, want, "tracked env")
    c = want["counts"][0]
    assert want["rows"][0] == 122 * N and c[SPAWN].sum() >= 3 * N * (122 // 9) and want["outside"].sum() == 0
    for role, agents in (("cop", (0, 1)), ("thief", (2,))):            # a seen and an unseen non-terminal row for each role
        seen, occ = c[SEEN][list(agents)].sum(), c[OCC][list(agents)].sum()
        assert 0 < seen < occ, (role, seen, occ)
    no_seen = {k: v.copy() for k, v in want.items()}
    no_seen["counts"][:, SEEN] = 0
    _same(small.position_tracker, no_seen, "position_exposure=False, rollout in chunks")
    assert small._tracked_rows["team_positions"].shape[0] == 7 and "obs_type" not in small._tracked_rows
    assert env._tracked_rows["obs_type"].shape[:2] == (60, N)
    # the stats are the summary of those counts; an explicit reset feeds nothing; off means no tracker
    s = env.position_stats()
    assert s[0]["rows"] == 122 * N and s[0]["agents"]["thief_0"]["seen"] == int(c[SEEN][2].sum())
    env.reset()
    _same(env.position_tracker, want, "after an explicit reset")
    assert env.position_stats(clear=True)[0]["rows"] == 122 * N and env.position_stats()[0]["rows"] == 0
    assert twin._positions is None and not hasattr(twin, "_tracked_rows")
    with pytest.raises(RuntimeError, match="track_positions"):
        twin.position_tracker
    for e in (env, small, twin):
        e.close()


def test_a_frame_skip_call_counts_one_row_per_slot():
    import torch
    from as_cops_and_thieves_amd.positions import PositionTracker
    N, cell = 63, 8
    env = _env(track_positions=cell)
    env.reset()
    rows = []
    for t in range(12):
        rows.append(_record(env, env.step_raw(env.random_actions(t), repeat=4)))
    torch.cuda.synchronize()
    env.check_errors()
    got = env.position_tracker.counts()
    assert got["rows"][0] == 12 * N and got["counts"].sum() - got["counts"][0, 1].sum() + got["outside"].sum() == 12 * N * 3
    cpu = PositionTracker(N, env.possible_agents, 2, tuple(int(v) for v in env._compiled[0].window), cell)
    rec = {k: torch.stack([r[k] for r in rows]) for k in rows[0]}
    cpu.update(rec["team_positions"], rec["terminated"], rec["obs_type"])
    _same(env.position_tracker, cpu.counts(), "repeat=4")
    assert int(rec["terminated"].sum()) > 0
    env.close()


def test_a_captured_step_replays_with_its_tracker_update_and_sees_set_groups():
    import torch
    N, cell = 63, 8
    env, twin = _env(track_positions=cell, position_groups=2), _env(track_positions=cell, position_groups=2)
    for e in (env, twin):
        e.reset()
    acts = env.random_actions(0).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up on the side stream, as torch's capture wants it
        env.step_raw(acts)
    torch.cuda.current_stream().wait_stream(side)
    twin.step_raw(acts)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.step_raw(acts)
    for _ in range(8):
        graph.replay()
    for _ in range(8):
        twin.step_raw(acts)
    torch.cuda.synchronize()
    _same(env.position_tracker, twin.position_tracker.counts(), "8 replays against 8 eager steps")
    assert env.position_tracker.counts()["rows"].tolist() == [9 * N, 0]
    groups = [1 if n % 2 else -1 for n in range(N)]
    for e in (env, twin):
        e.position_tracker.set_groups(groups)
    for _ in range(3):
        graph.replay()
        twin.step_raw(acts)
    torch.cuda.synchronize()
    _same(env.position_tracker, twin.position_tracker.counts(), "set_groups between replays")
    assert env.position_tracker.counts()["rows"].tolist() == [9 * N, 3 * (N // 2)]
    for e in (env, twin):
        e.check_errors()
        e.close()


def test_evaluate_league_counts_the_first_episode_of_every_slot_per_segment():
    import torch
    from as_cops_and_thieves_amd.selfplay.actor import LeagueActor
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_league
    env = _env(N=8, seed=5, track_positions=8, position_groups=2, track_episodes=True)
    league = LeagueActor.from_env(env, 3, fused="kernel", seed=2)
    league.set_matchups([(0, 4, {"cop_0": 0, "cop_1": 1, "thief_0": 2}), (4, 8, {"cop_0": 1, "cop_1": 0, "thief_0": "random"})])
    env.episode_tracker.set_quota(1)                        # the episode tracker, too, counts the first episode of every slot
    torch.manual_seed(1)
    res = evaluate_league(env, league, positions=True)
    env.check_errors()
    lengths = env.episode_tracker.per_slot()["len_sum"].cpu()
    assert torch.equal(lengths.to(torch.int32), res["length"].cpu()) and int(lengths.min()) >= 1
    got = env.position_tracker.counts()
    assert got["rows"].tolist() == [int(lengths[:4].sum()), int(lengths[4:].sum())]
    assert got["done"].tolist() == [1] * 8
    assert [g["rows"] for g in res["positions"]] == got["rows"].tolist()
    assert got["counts"][:, 2].sum(axis=(1, 2, 3)).tolist() == [4 * 3, 4 * 3]        # one spawn per slot and agent: the terminal row
    env.close()
