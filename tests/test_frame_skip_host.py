"""Frame skip, the parts that need no device: the new entry in header, library and ctypes mirror; argument checks that come before any device call."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_step_repeat_is_declared_exported_and_mirrored_alike():
    import ctypes as C
    from as_cops_and_thieves_amd import _native
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_sim.h").read_text(), flags=re.S)
    m = re.search(r"int\s+cat_step_repeat\s*\(([^)]*)\)\s*;", text)
    assert m, "include/cat_sim.h does not declare cat_step_repeat"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["cat_sim *sim", "int k", "const int32_t *actions", "int auto_reset", "const cat_outputs *out", "int32_t *ticks", "void *stream"]
    assert "cat_step_repeat" in _native.EXPORTED_SYMBOLS
    _native.build()
    L = _native.lib()
    fn = L.cat_step_repeat
    assert fn.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] and fn.restype == C.c_int
    assert fn(None, 4, None, 1, None, None, None) == -6            # no handle: refused before any device call
    assert _native.MAX_ROLLOUT_TICKS == int(re.search(r"#define CAT_MAX_ROLLOUT_TICKS (\d+)", text).group(1))


@pytest.mark.parametrize("bad", [0, -1, 2.5, "3", True, None, 65537])
def test_repeat_counts_are_validated_before_a_device_is_touched(bad):
    from as_cops_and_thieves_amd.environments import VecCopsEnv, check_repeat
    from as_cops_and_thieves_amd.maps import load_preset
    with pytest.raises(ValueError):
        check_repeat(bad)
    with pytest.raises(ValueError, match="frame_skip"):
        VecCopsEnv(load_preset("squarinth"), 4, frame_skip=bad)     # raises on the argument: no sim is created
    if bad is not None:                                                   # (None = "the env's default" for a call)
        env = object.__new__(VecCopsEnv)                                 # no device behind it: the check must come first
        with pytest.raises(ValueError):
            env.step(None, repeat=bad)
        env.frame_skip = 1
        with pytest.raises(ValueError):
            env.step_raw(None, repeat=bad)


def test_valid_repeat_counts_pass():
    import numpy as np
    from as_cops_and_thieves_amd.environments import check_repeat
    assert check_repeat(1) == 1 and check_repeat(np.int64(4)) == 4 and check_repeat(65536) == 65536


# ---------------------------------------------------------------------------------------------- the tracker's update for windows
def test_episode_windows_entry_is_declared_exported_and_mirrored_alike():
    import ctypes as C
    from as_cops_and_thieves_amd import _learn_native as ln
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_episodes.h").read_text(), flags=re.S)
    m = re.search(r"int\s+cat_episode_windows_update\s*\(([^)]*)\)\s*;", code)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["const cat_episode_windows_args *a", "void *stream"]
    body = re.search(r"typedef struct cat_episode_windows_args \{(.*?)\} cat_episode_windows_args;", code, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["cat_episodes_update_args u", "const int32_t *ticks"]
    assert [f[0] for f in ln.EpisodeWindows._fields_] == ["u", "ticks"] and ln.EpisodeWindows._fields_[0][1] is ln.EpisodesUpdate
    assert C.sizeof(ln.EpisodeWindows) == C.sizeof(ln.EpisodesUpdate) + 8
    assert ln.EPISODE_WINDOWS_SYMBOLS == ("cat_episode_windows_update",)
    ln.build()
    L = ln.lib()
    fn = L.cat_episode_windows_update
    assert fn.argtypes == [C.c_void_p, C.c_void_p] and fn.restype == C.c_int
    assert fn(None, None) == -1 and b"dimensions" in L.cat_episodes_last_error()           # refused before any device call
    assert fn(C.byref(ln.EpisodeWindows(ln.EpisodesUpdate(1, 4, 2, 10), None)), None) == -1 and b"NULL" in L.cat_episodes_last_error()


def _episode_streams(n_slots, agents, lengths_per_slot, rng):
    """Tick streams [T, N, ...] in which slot n plays episodes of the given lengths back to back (the last one may stay open)."""
    import numpy as np
    T = max(sum(ls) for ls in lengths_per_slot)
    reward = rng.standard_normal((T, n_slots, agents)).astype(np.float32)
    term = np.zeros((T, n_slots), np.uint8); trunc = np.zeros((T, n_slots), np.uint8); win = np.full((T, n_slots), -1, np.int8)
    for n, ls in enumerate(lengths_per_slot):
        t = 0
        for i, L in enumerate(ls):
            t += L
            if t < T or sum(ls) == T and i < len(ls) - 1 or (n % 2 == 0 and t == T):
                term[t - 1, n] = 1
                trunc[t - 1, n] = (i + n) % 3 == 0
                win[t - 1, n] = 1 if trunc[t - 1, n] else (i + n) % 2
    return reward, term, trunc, win


def test_tracker_fed_windows_equals_tracker_fed_tick_by_tick():
    """Windows of (3, 1, 4, ...) ticks, cut where an episode ends (the hold rule), against the same ticks one by one: lengths,
    histogram, outcomes and counts are equal; a return is the f64 sum of the fp32 window sums in window order."""
    import numpy as np
    import torch
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    rng = np.random.default_rng(5)
    N, A, MSC = 5, 3, 9
    lengths = [[9, 2, 7, 9, 3], [1, 1, 9, 5, 9, 5], [4, 9, 9, 8], [9, 9, 9, 3], [2, 3, 5, 7, 9, 4]]
    reward, term, trunc, win = _episode_streams(N, A, lengths, rng)
    T = reward.shape[0]
    by_tick = EpisodeTracker(N, ["cop_0", "cop_1", "thief_0"], MSC)
    by_tick.update(*(torch.from_numpy(x) for x in (reward, term, trunc, win)))
    # cut every slot's stream into windows of at most k ticks, k cycling through (3, 1, 4, 2), ending early at a terminal tick
    ks, pos, rows = (3, 1, 4, 2), [0] * N, []
    d = 0
    while any(p < T for p in pos):
        k = ks[d % len(ks)]
        row = {"reward": np.zeros((N, A), np.float32), "term": np.zeros(N, np.uint8), "trunc": np.zeros(N, np.uint8),
               "win": np.full(N, -1, np.int8), "ticks": np.ones(N, np.int32), "live": np.zeros(N, bool)}
        for n in range(N):
            if pos[n] >= T:
                continue
            j, acc = 0, None
            while True:
                r = reward[pos[n] + j, n]
                acc = r.copy() if acc is None else (acc + r).astype(np.float32)          # the fp32 left fold
                if term[pos[n] + j, n] or j + 1 == k or pos[n] + j + 1 == T:
                    break
                j += 1
            last = pos[n] + j
            row["reward"][n], row["term"][n], row["trunc"][n], row["win"][n] = acc, term[last, n], trunc[last, n], win[last, n]
            row["ticks"][n], row["live"][n] = j + 1, True
            pos[n] = last + 1
        rows.append(row)
        d += 1
    assert {int(t) for r in rows for t in r["ticks"][r["live"]]} == {1, 2, 3, 4}
    by_window = EpisodeTracker(N, ["cop_0", "cop_1", "thief_0"], MSC)
    want_run = np.zeros((N, A)); want_sum = np.zeros((N, A)); want_sq = np.zeros((N, A))
    for r in rows:          # slots whose stream is over are fed nothing: a tracker per live set would do; here a zero-tick row cannot be
        live = r["live"]    # expressed, so such slots are parked by feeding them through a second tracker that is thrown away
        keep = {k: v.numpy().copy() for k, v in by_window.state.items()}
        by_window.update(torch.from_numpy(r["reward"]), torch.from_numpy(r["term"]), torch.from_numpy(r["trunc"]), torch.from_numpy(r["win"]),
                         ticks=torch.from_numpy(r["ticks"]))
        for k, v in by_window.state.items():
            if k != "len_hist":
                v.numpy()[~live] = keep[k][~live]
        for n in np.nonzero(live)[0]:
            want_run[n] += r["reward"][n].astype(np.float64)
            if r["term"][n]:
                want_sum[n] += want_run[n]; want_sq[n] += want_run[n] * want_run[n]; want_run[n] = 0.0
    assert all(not (r["term"][~r["live"]]).any() for r in rows)      # parked slots never end an episode: the histogram needs no parking
    a, b = by_tick.summary(), by_window.summary()
    for key in ("episodes", "cop_wins", "thief_wins", "timeouts", "min_length", "max_length", "mean_length", "length_hist"):
        assert a[key] == b[key], key
    assert a["episodes"] >= 20 and a["timeouts"] > 0 and a["cop_wins"] > 0 and sum(x > 0 for x in a["length_hist"]) >= 5
    for key in ("len_run", "finished", "len_sum", "len_min", "len_max"):
        assert np.array_equal(by_tick.state[key].numpy(), by_window.state[key].numpy()), key
    # the documented summation rule, bit for bit; and it is close to, but not the same arithmetic as, the tick-by-tick f64 sum
    assert np.array_equal(by_window.state["ret_sum"].numpy(), want_sum) and np.array_equal(by_window.state["ret_sq"].numpy(), want_sq)
    assert np.array_equal(by_window.state["ret_run"].numpy(), want_run)
    assert np.allclose(by_window.state["ret_sum"].numpy(), by_tick.state["ret_sum"].numpy(), rtol=0, atol=1e-5)


def test_tracker_refuses_ticks_of_the_wrong_shape():
    import torch
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    tr = EpisodeTracker(4, ["cop_0", "thief_0"], 10)
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError, match="ticks"):
        tr.update(z(4, 2, dt=torch.float32), z(4), z(4), z(4, dt=torch.int8), ticks=torch.ones(5, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("bad", [0, -2, 2.5, True, None])
def test_trainer_config_validates_frame_skip(bad):
    from as_cops_and_thieves_amd.selfplay.mappo import TrainerConfig
    with pytest.raises(ValueError, match="frame_skip"):
        TrainerConfig(frame_skip=bad)
    assert TrainerConfig().frame_skip == 1 and TrainerConfig(frame_skip=3).frame_skip == 3


def test_evaluations_validate_frame_skip_before_touching_the_env():
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_agents, evaluate_agents_tracked, evaluate_league

    class Who:
        N, device, agents, table, segments = 2, "cpu", ["cop_0"], (), ()

    class Env:
        num_envs = 2

        def __getattr__(self, name):
            raise AssertionError(f"the env was touched ({name}) before frame_skip was checked")
    for fn, args in ((evaluate_agents, (Env(), None, 1)), (evaluate_agents_tracked, (Env(), None, 1)), (evaluate_league, (Env(), Who()))):
        with pytest.raises(ValueError, match="frame_skip"):
            fn(*args, **({"actor": Who()} if fn is not evaluate_league else {}), frame_skip=0)


def _skip_env_class():
    import numpy as np
    import torch
    from tests.fake_env import OracleVecEnv

    class SkipEnv(OracleVecEnv):
        """The CPU stand-in with ``step(actions, repeat=)``: up to ``repeat`` held-action ticks per slot, stopped where the slot's episode
        ends (the slot is then reset and parked), rewards folded in fp32, ``infos["ticks"]``.  Records every call."""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls = []

        def step(self, actions, repeat=1):
            acts = np.ascontiguousarray(np.asarray(actions, dtype=np.int32))
            self.calls.append(repeat)
            N = self.num_envs
            live = np.ones(N, bool)
            total = np.zeros((N, len(self.possible_agents)), np.float32)
            ticks = np.zeros(N, np.int32)
            flags = {k: None for k in ("terminated", "truncated", "winner")}
            for j in range(repeat):
                before = self.sim.get_state()
                out = self.sim.step(acts)
                o = {k: out[k].copy() for k in ("reward", "terminated", "truncated", "winner")}
                self.sim.reset(mask=(o["terminated"] != 0) & live)
                after = self.sim.get_state()
                self.sim.set_state(**{k: np.where(live.reshape((N,) + (1,) * (np.asarray(v).ndim - 1)), after[k], np.asarray(v))
                                      for k, v in before.items()})               # held slots do not advance
                total[live] = total[live] + o["reward"][live] if j else o["reward"][live]
                ticks[live] += 1
                for k in flags:
                    flags[k] = o[k].copy() if flags[k] is None else np.where(live, o[k], flags[k])
                live = live & (o["terminated"] == 0)
            self.last_rewards = total.copy()
            rew = {a: torch.from_numpy(total[:, i].copy()) for i, a in enumerate(self.possible_agents)}
            term = torch.from_numpy(flags["terminated"].astype(bool)); trunc = torch.from_numpy(flags["truncated"].astype(bool))
            infos = {"winner": torch.from_numpy(flags["winner"].copy()), "ticks": torch.from_numpy(ticks.copy())}
            self.last_ticks = ticks.copy()
            return self._obs(), rew, {a: term for a in self.possible_agents}, {a: trunc for a in self.possible_agents}, infos
    return SkipEnv


def test_trainer_forwards_repeat_sums_nothing_itself_and_counts_env_ticks():
    import numpy as np
    import torch
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    SkipEnv = _skip_env_class()
    cmap = load_preset("squarinth").compile()
    rc = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0, kl_threshold=0.0)
    env = SkipEnv(cmap, 6, num_rays=16, max_step_count=5, seed=2)
    tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, TrainerConfig(horizon=4, timesteps=8, frame_skip=3))
    seen_rewards, seen_ticks = [], []
    step = env.step

    def spy(actions, repeat=1):
        res = step(actions, repeat=repeat)
        seen_rewards.append(env.last_rewards.copy()); seen_ticks.append(env.last_ticks.copy())
        return res
    env.step = spy
    tr.collect()
    assert env.calls == [3, 3, 3, 3] and tr.timestep == 4                    # a timestep is a decision
    rl = tr.roles["cop+thief"]
    got = rl.buf["rew"].numpy()                                                # [G, T, N]
    want = np.stack(seen_rewards).transpose(2, 0, 1)                           # the env's window sums, untouched
    assert got.dtype == np.float32 and np.array_equal(got, want)
    total = int(np.stack(seen_ticks).sum())
    assert any((t < 3).any() for t in seen_ticks) and any((t == 3).any() for t in seen_ticks)    # 5-tick episodes end inside windows
    assert tr.read_stats()["env_ticks"] == total
    tr.collect()
    assert tr.read_stats()["env_ticks"] == int(np.stack(seen_ticks).sum()) > total and env.calls == [3] * 8
    # frame_skip = 1: the env is called as before this option existed (no keyword), and env_ticks is N per tick
    plain = SkipEnv(cmap, 6, num_rays=16, max_step_count=5, seed=2)
    plain.step = lambda actions: step.__func__(plain, actions)                # a step() without the keyword: it must not be passed
    tr1 = MAPPOTrainer(plain, {"cop": rc, "thief": rc}, TrainerConfig(horizon=4, timesteps=8))
    tr1.collect()
    assert plain.calls == [1] * 4 and tr1.read_stats()["env_ticks"] == 6 * 4
