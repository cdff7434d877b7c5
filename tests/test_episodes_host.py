"""Episode accounting on the host (include/cat_episodes.h, as_cops_and_thieves_amd/episodes.py): the CPU form of ``EpisodeTracker``
against a plain per-slot Python loop written here, bit for bit; chunking invariance; header <-> library <-> ctypes mirror; the
tracked evaluation against ``evaluate_agents`` and the self-play loop with both options on the CPU stand-in env."""
import ctypes as C
import dataclasses
import json
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd.episodes import EpisodeTracker
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
from as_cops_and_thieves_amd.selfplay.self_play import TrainingConfig, evaluate_agents, evaluate_agents_tracked, run_self_play
from tests.fake_env import OracleVecEnv

warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")
ROOT = Path(__file__).resolve().parents[1]
INT32_MAX = 2 ** 31 - 1
SLOT_FIELDS = ("ret_run", "len_run", "finished", "cop_wins", "thief_wins", "timeouts", "len_sum", "len_min", "len_max", "ret_sum", "ret_sq")


# ---------------------------------------------------------------------------------------------- the restatement of this test
class LoopTracker:
    """include/cat_episodes.h read literally: one slot at a time, one tick at a time, Python floats (IEEE doubles; ``a * b`` then
    ``+`` are two roundings)."""

    def __init__(self, N, A, msc):
        self.N, self.A, self.msc, self.quota = N, A, msc, None
        self.ret_run = [[0.0] * A for _ in range(N)]
        self.len_run = [0] * N
        self.clear()

    def clear(self):
        N, A = self.N, self.A
        self.finished, self.cop_wins, self.thief_wins, self.timeouts, self.len_sum, self.len_max = ([0] * N for _ in range(6))
        self.len_min = [INT32_MAX] * N
        self.ret_sum, self.ret_sq = [[0.0] * A for _ in range(N)], [[0.0] * A for _ in range(N)]
        self.len_hist = [0] * 64

    def abandon(self, mask=None):
        for n in range(self.N):
            if mask is None or mask[n]:
                self.ret_run[n], self.len_run[n] = [0.0] * self.A, 0

    def update(self, reward, terminated, truncated, winner):
        for n in range(self.N):
            for t in range(reward.shape[0]):
                for a in range(self.A):
                    self.ret_run[n][a] += float(reward[t, n, a])
                self.len_run[n] += 1
                if terminated[t, n]:
                    if self.quota is None or self.finished[n] < self.quota[n]:
                        L = self.len_run[n]
                        self.finished[n] += 1
                        self.cop_wins[n] += int(winner[t, n] == 0)
                        self.thief_wins[n] += int(winner[t, n] == 1)
                        self.timeouts[n] += int(truncated[t, n] != 0)
                        self.len_sum[n] += L
                        self.len_min[n], self.len_max[n] = min(self.len_min[n], L), max(self.len_max[n], L)
                        for a in range(self.A):
                            self.ret_sum[n][a] += self.ret_run[n][a]
                            self.ret_sq[n][a] += self.ret_run[n][a] * self.ret_run[n][a]
                        self.len_hist[min(63, (L - 1) * 64 // self.msc)] += 1
                    self.ret_run[n], self.len_run[n] = [0.0] * self.A, 0

    @staticmethod
    def tree(x):
        x = np.asarray(x, dtype=np.float64)
        P = 1
        while P < x.shape[0]:
            P *= 2
        x = np.concatenate([x, np.zeros((P - x.shape[0],) + x.shape[1:])])
        while x.shape[0] > 1:
            h = x.shape[0] // 2
            x = x[:h] + x[h:]
        return x[0]

    def block(self):
        return {"episodes": sum(self.finished), "cop_wins": sum(self.cop_wins), "thief_wins": sum(self.thief_wins), "timeouts": sum(self.timeouts),
                "open_slots": 0 if self.quota is None else sum(f < q for f, q in zip(self.finished, self.quota)),
                "len_sum": sum(self.len_sum), "len_min": min(self.len_min), "len_max": max(self.len_max),
                "ret_sum": self.tree(self.ret_sum).tolist(), "ret_sq": self.tree(self.ret_sq).tolist(), "len_hist": list(self.len_hist)}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def assert_same(tr: EpisodeTracker, ref: LoopTracker, ctx=""):
    st = tr.per_slot()
    for k in SLOT_FIELDS:
        got, want = st[k].numpy(), np.asarray(getattr(ref, k))
        if got.dtype == np.float64:
            assert bits(got) == bits(want), (ctx, k)
        else:
            assert got.tolist() == want.tolist(), (ctx, k)
    got, want = tr.summary_block(), ref.block()
    assert set(got) == set(want)
    for k in want:
        assert (bits(got[k]) == bits(want[k])) if k in ("ret_sum", "ret_sq") else (got[k] == want[k]), (ctx, k, got[k], want[k])


def feed(tr, reward, terminated, truncated, winner, cuts=None):
    T = reward.shape[0]
    cuts = [0, T] if cuts is None else cuts
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        tr.update(*(torch.from_numpy(np.ascontiguousarray(x[lo:hi])) for x in (reward, terminated, truncated, winner)))


def random_stream(rng, T, N, A, p_end=0.15):
    """Rewards of mixed magnitude (the order of the f64 adds shows in the last bits), ends at random, a third of them timeouts."""
    mag = rng.choice([1e-3, 1.0, 1e4, 3e7], size=(T, N, A))
    reward = (rng.standard_normal((T, N, A)) * mag).astype(np.float32)
    terminated = (rng.random((T, N)) < p_end).astype(np.uint8)
    truncated = (terminated * (rng.random((T, N)) < 0.33)).astype(np.uint8)
    winner = np.where(terminated == 0, -1, np.where(truncated == 1, 1, rng.integers(0, 2, (T, N)))).astype(np.int8)
    return reward, terminated, truncated, winner


# ---------------------------------------------------------------------------------------------- 1. tracker == loop
def test_hand_made_stream_with_known_answers():
    """Two slots, two agents, max_step_count 4.  Slot 0: a capture on tick 0, then a capture on the very next tick, then a timeout
    after 4 ticks.  Slot 1: nothing ends."""
    N, A, T = 2, 2, 6
    reward = np.zeros((T, N, A), np.float32)
    reward[:, 0, 0] = [1.0, 2.0, 0.5, 0.5, 0.5, 0.5]
    reward[:, 0, 1] = [-1.0, -2.0, 0.25, 0.25, 0.25, 0.25]
    reward[:, 1, 0] = 1.0
    terminated = np.zeros((T, N), np.uint8); terminated[[0, 1, 5], 0] = 1
    truncated = np.zeros((T, N), np.uint8); truncated[5, 0] = 1
    winner = np.full((T, N), -1, np.int8); winner[[0, 1], 0] = 0; winner[5, 0] = 1
    tr = EpisodeTracker(N, ["cop_0", "thief_0"], 4)
    feed(tr, reward, terminated, truncated, winner)
    s = tr.summary()
    assert (s["episodes"], s["cop_wins"], s["thief_wins"], s["timeouts"], s["open_slots"]) == (3, 2, 1, 1, 0)
    assert (s["min_length"], s["max_length"], s["mean_length"], s["cop_win_rate"]) == (1, 4, 2.0, 2 / 3)
    assert s["mean_return/cop_0"] == (1.0 + 2.0 + 2.0) / 3 and s["mean_return/thief_0"] == (-1.0 - 2.0 + 1.0) / 3
    assert abs(s["std_return/cop_0"] - np.std([1.0, 2.0, 2.0])) < 1e-12
    hist = [0] * 64; hist[0] = 2; hist[48] = 1            # lengths 1, 1 -> bin 0; length 4 -> (4 - 1) * 64 // 4 = 48
    assert s["length_hist"] == hist
    st = tr.per_slot()
    assert st["len_run"].tolist() == [0, 6] and st["ret_run"].tolist() == [[0.0, 0.0], [6.0, 0.0]] and st["finished"].tolist() == [3, 0]
    assert st["len_min"].tolist() == [1, INT32_MAX] and st["len_sum"].tolist() == [6, 0]
    ref = LoopTracker(N, A, 4)
    ref.update(reward, terminated, truncated, winner)
    assert_same(tr, ref)


@pytest.mark.parametrize("quota", [0, 1, 3])
def test_quota_counts_the_first_episodes_and_restarts_the_rest(quota):
    rng = np.random.default_rng(quota)
    N, A, T = 5, 2, 60
    stream = random_stream(rng, T, N, A, p_end=0.3)
    tr, ref = EpisodeTracker(N, ["cop_0", "thief_0"], 20), LoopTracker(N, A, 20)
    tr.set_quota(quota); ref.quota = [quota] * N
    feed(tr, *stream); ref.update(*stream)
    assert_same(tr, ref)
    ended = stream[1].sum(0)
    assert tr.per_slot()["finished"].tolist() == np.minimum(ended, quota).tolist()
    assert tr.summary()["open_slots"] == int((ended < quota).sum())
    # per-slot quotas from a tensor; None lifts the limit again
    q = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32)
    tr.clear(); ref.clear(); tr.set_quota(q); ref.quota = q.tolist()
    feed(tr, *stream); ref.update(*stream)
    assert_same(tr, ref, "tensor quota")
    buf = tr.per_slot()["quota"].data_ptr()                  # one buffer for the tracker's life: a captured update launch keeps reading it
    tr.set_quota(2); tr.set_quota(q)
    assert tr.per_slot()["quota"].data_ptr() == buf and tr.per_slot()["quota"].tolist() == q.tolist()
    tr.set_quota(None); ref.quota = None
    assert tr.quota is None and tr._quota.data_ptr() == buf
    feed(tr, *stream); ref.update(*stream)
    assert_same(tr, ref, "no quota")


def test_abandon_and_clear():
    rng = np.random.default_rng(11)
    N, A = 7, 3
    names = ["cop_0", "cop_1", "thief_0"]
    tr, ref = EpisodeTracker(N, names, 9), LoopTracker(N, A, 9)
    a, b, c = (random_stream(rng, 20, N, A) for _ in range(3))
    feed(tr, *a); ref.update(*a)
    mask = np.array([1, 0, 0, 1, 0, 1, 0], np.uint8)
    tr.abandon(torch.from_numpy(mask)); ref.abandon(mask)
    assert_same(tr, ref, "masked abandon")
    assert tr.per_slot()["len_run"][mask == 1].tolist() == [0, 0, 0]
    feed(tr, *b); ref.update(*b)
    tr.clear(); ref.clear()                                 # the totals go, the running values stay
    assert tr.summary()["episodes"] == 0 and tr.summary()["min_length"] == 0 and sum(tr.summary()["length_hist"]) == 0
    assert_same(tr, ref, "clear")
    assert tr.per_slot()["len_run"].sum() > 0
    feed(tr, *c); ref.update(*c)
    tr.abandon(); ref.abandon()
    assert_same(tr, ref, "abandon all")
    assert tr.per_slot()["len_run"].sum() == 0 and float(tr.per_slot()["ret_run"].abs().sum()) == 0.0


@pytest.mark.parametrize("N,A", [(1, 2), (7, 3), (37, 5), (130, 3), (1500, 2)])
def test_random_streams_equal_the_loop_bit_for_bit(N, A):
    rng = np.random.default_rng(1000 * N + A)
    T = 70 if N < 200 else 24
    names = [f"cop_{i}" for i in range(A - 1)] + ["thief_0"]
    tr, ref = EpisodeTracker(N, names, 25), LoopTracker(N, A, 25)
    stream = random_stream(rng, T, N, A)
    feed(tr, *stream); ref.update(*stream)
    assert_same(tr, ref)
    s = tr.summary()
    assert s["episodes"] == int(stream[1].sum()) and sum(s["length_hist"]) == s["episodes"] and s["cop_wins"] + s["thief_wins"] == s["episodes"]
    if N in (37, 130):
        assert s["length_hist"][63] > 0        # lengths beyond max_step_count land in the last bin


def test_the_order_of_the_slot_sum_is_the_halving_tree():
    """The totals are NOT numpy's own sum of the slots (pairwise in blocks) nor a running sum: with returns of mixed magnitude the
    three differ in the last bits, and the tracker gives the tree's."""
    rng = np.random.default_rng(5)
    N, A = 1000, 2
    tr = EpisodeTracker(N, ["cop_0", "thief_0"], 50)
    stream = random_stream(rng, 40, N, A)
    feed(tr, *stream)
    per = tr.per_slot()["ret_sum"].numpy()
    tree = LoopTracker.tree(per)
    assert bits(tr.summary_block()["ret_sum"]) == bits(tree)
    running = np.zeros(A)
    for row in per:
        running = running + row
    assert bits(running) != bits(tree)


# ---------------------------------------------------------------------------------------------- 2. chunking invariance
def test_chunking_invariance():
    rng = np.random.default_rng(77)
    N, A, T = 45, 3, 50
    stream = random_stream(rng, T, N, A)
    names = ["cop_0", "cop_1", "thief_0"]
    whole, single, ragged = (EpisodeTracker(N, names, 30) for _ in range(3))
    for tr in (whole, single, ragged):
        tr.set_quota(torch.arange(N, dtype=torch.int32) % 6)
    feed(whole, *stream)
    for t in range(T):                                     # [N, ...] calls, as step / step_raw make them
        single.update(*(torch.from_numpy(x[t].copy()) for x in stream))
    feed(ragged, *stream, cuts=[0, 1, 2, 9, 10, 33, 49, 50])
    a = whole.per_slot()
    for other in (single, ragged):
        b = other.per_slot()
        for k in SLOT_FIELDS + ("len_hist",):
            assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k
        assert whole.summary() == other.summary()
    assert whole.summary()["episodes"] > 20


def test_update_refuses_wrong_shapes():
    tr = EpisodeTracker(4, ["cop_0", "thief_0"], 10)
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError):
        tr.update(z(4, 3, dt=torch.float32), z(4), z(4), z(4, dt=torch.int8))
    with pytest.raises(ValueError):
        tr.update(z(2, 4, 2, dt=torch.float32), z(2, 4), z(2, 5), z(2, 4, dt=torch.int8))
    with pytest.raises(ValueError):
        EpisodeTracker(4, ["a"] * 9, 10)


# ---------------------------------------------------------------------------------------------- 3. header <-> library <-> ctypes
def test_episodes_header_matches_the_library_and_the_ctypes_mirror():
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.build()
    L = ln.lib()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_episodes.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cat_episodes_[a-z_0-9]+)\s*\(", code)))
    assert set(declared) == set(ln.EPISODES_SYMBOLS) and len(declared) == 4 and all(hasattr(L, s) for s in declared)
    assert L.cat_episodes_abi_version() == 1
    structs = {"cat_episodes_state": ln.EpisodesState, "cat_episodes_update_args": ln.EpisodesUpdate,
               "cat_episodes_summary_block": ln.EpisodesSummaryBlock, "cat_episodes_summary_args": ln.EpisodesSummary}
    for struct, cls in structs.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
        body = re.sub(r"\[[^\]]*\]", "", body)                                  # array extents
        names = [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    assert C.sizeof(ln.EpisodesSummaryBlock) == 6 * 8 + 2 * 4 + 2 * 8 * 8 and C.sizeof(ln.EpisodesState) == 12 * 8
    assert (ROOT / "as_cops_and_thieves_amd" / "csrc" / "cat_episodes.hip") in ln.SOURCES and (ROOT / "include" / "cat_episodes.h") in ln.HEADERS


def test_episodes_entries_refuse_bad_arguments_before_touching_a_device():
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    assert L.cat_episodes_update(None, None) == -1
    assert L.cat_episodes_update(C.byref(ln.EpisodesUpdate()), None) == -1 and b"dimensions" in L.cat_episodes_last_error()
    for T, N, A, msc in ((0, 4, 2, 10), (65537, 4, 2, 10), (1, 0, 2, 10), (1, 4, 0, 10), (1, 4, 9, 10), (1, 4, 2, 0)):
        a = ln.EpisodesUpdate(T, N, A, msc)
        assert L.cat_episodes_update(C.byref(a), None) == -1 and b"dimensions" in L.cat_episodes_last_error(), (T, N, A, msc)
    a = ln.EpisodesUpdate(1, 4, 2, 10)                       # dimensions fine, every buffer NULL
    assert L.cat_episodes_update(C.byref(a), None) == -1 and b"NULL" in L.cat_episodes_last_error()
    assert L.cat_episodes_summary(None, None) == -1
    assert L.cat_episodes_summary(C.byref(ln.EpisodesSummary(0, 2)), None) == -1 and b"dimensions" in L.cat_episodes_last_error()
    assert L.cat_episodes_summary(C.byref(ln.EpisodesSummary(4, 9)), None) == -1
    assert L.cat_episodes_summary(C.byref(ln.EpisodesSummary(4, 2)), None) == -1 and b"NULL" in L.cat_episodes_last_error()


# ---------------------------------------------------------------------------------------------- 4. / 5. evaluation and self-play
class TrackedOracleVecEnv(OracleVecEnv):
    """The CPU stand-in env with the surface ``VecCopsEnv(track_episodes=True)`` adds: an ``episode_tracker`` fed on every step."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.episode_tracker = EpisodeTracker(self.num_envs, self.possible_agents, self.max_step_count)

    def reset(self, seed=None, options=None):
        self.episode_tracker.abandon()
        return super().reset(seed, options)

    def step(self, actions):
        obs, rew, terms, truncs, infos = super().step(actions)
        first = self.possible_agents[0]
        self.episode_tracker.update(torch.stack([rew[a] for a in self.possible_agents], dim=1), terms[first], truncs[first], infos["winner"])
        return obs, rew, terms, truncs, infos

    def episode_stats(self, clear=False):
        stats = self.episode_tracker.summary()
        if clear:
            self.episode_tracker.clear()
        return stats

    def get_env_state(self, out=None):
        return {k: torch.from_numpy(v) for k, v in self.sim.get_state().items()}

    def set_env_state(self, **arrays):
        self.sim.set_state(**{k: np.asarray(v) for k, v in arrays.items()})


CMAP = load_preset("squarinth").compile()
RC = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=4, learning_starts=8, kl_threshold=0.0)
TC = TrainerConfig(horizon=4, timesteps=16, policy_freeze_duration=8, opponent_freeze_duration=8)
PLAIN = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=12, seed=s)
TRACKED = lambda n, s: TrackedOracleVecEnv(CMAP, n, num_rays=16, max_step_count=12, seed=s)
# 400-tick episodes: with untrained networks about a quarter of the episodes end in a capture, on different ticks from slot to slot
PLAIN_LONG = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=400, seed=s)
TRACKED_LONG = lambda n, s: TrackedOracleVecEnv(CMAP, n, num_rays=16, max_step_count=400, seed=s)


def sim_state_bytes(env):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in env.sim.get_state().items()}


@pytest.mark.parametrize("n_episodes,poll_every", [(24, 1), (24, 5), (24, 32), (10, 7), (24, 150)])
def test_tracked_evaluation_equals_evaluate_agents(n_episodes, poll_every):
    """Three evaluations in a row on ONE env, without reseeding in between, as the self-play loop makes them: each must give what
    ``evaluate_agents`` gives, and leave the generators and the env where it leaves them -- else the next one starts elsewhere."""
    runs = []
    for factory, fn, kw in ((PLAIN_LONG, evaluate_agents, {}), (TRACKED_LONG, evaluate_agents_tracked, {"poll_every": poll_every})):
        env = factory(24, 5)
        runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=2)
        torch.manual_seed(1234)
        seen = []
        for _ in range(3):
            res = fn(env, runner, n_episodes, **kw)
            seen.append((res, torch.get_rng_state().numpy().tobytes(), sim_state_bytes(env)))
        runs.append(seen)
    for k, ((res_a, rng_a, st_a), (res_b, rng_b, st_b)) in enumerate(zip(*runs)):
        assert res_a == res_b, (k, res_a, res_b)
        assert abs(sum(res_b) - 1.0) < 1e-9
        assert rng_a == rng_b, k                             # it stops drawing where evaluate_agents stops
        for key in st_a:
            assert st_a[key] == st_b[key], (k, key)         # and the env stands where evaluate_agents leaves it
    # the comparison is not one of (0, 1) with (0, 1): both sides win episodes, and the slots end on different ticks
    assert all(res[0] > 0 and res[1] > 0 for res, _, _ in runs[1]), [r for r, _, _ in runs[1]]
    assert len({res for res, _, _ in runs[1]}) > 1
    s = env.episode_tracker.summary()
    assert s["episodes"] == n_episodes and s["open_slots"] == 0 and s["cop_wins"] >= 1 and s["thief_wins"] >= 1
    assert s["min_length"] < s["max_length"]
    assert env.episode_tracker.per_slot()["finished"].tolist() == [1] * n_episodes + [0] * (24 - n_episodes)


def test_tracked_evaluation_with_random_roles_equals_evaluate_agents():
    out = []
    for factory, fn in ((PLAIN, evaluate_agents), (TRACKED, evaluate_agents_tracked)):
        env = factory(6, 9)
        runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=4)
        torch.manual_seed(99)
        out.append(fn(env, runner, 5, random_roles=("thief",)))
    assert out[0] == out[1]


@pytest.mark.parametrize("n_episodes,poll_every", [(15, 4), (20, 32)])
def test_tracked_evaluation_plays_several_episodes_per_slot(n_episodes, poll_every):
    env = TRACKED(6, 5)
    runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=2)
    cop, thief = evaluate_agents_tracked(env, runner, n_episodes, poll_every=poll_every)
    s = env.episode_tracker.summary()
    assert s["episodes"] == n_episodes and s["open_slots"] == 0 and s["cop_wins"] + s["thief_wins"] == n_episodes
    assert abs(cop + thief - 1.0) < 1e-9 and cop == s["cop_wins"] / n_episodes
    want = [n_episodes // 6 + (n < n_episodes % 6) for n in range(6)]
    assert env.episode_tracker.per_slot()["finished"].tolist() == want
    assert s["timeouts"] <= s["thief_wins"] and s["max_length"] <= 12 and sum(s["length_hist"]) == n_episodes


def test_trainer_reports_the_episodes_of_its_train_call():
    digests = []
    for flag in (False, True):
        env = TRACKED(8, 1)
        tr = MAPPOTrainer(env, {"cop": RC, "thief": RC}, dataclasses.replace(TC, episode_stats=flag), seed=0)
        stats = tr.train(16)
        digests.append(tr.param_digest())
        assert ("episodes" in stats) == flag
    assert digests[0] == digests[1]
    assert stats["episodes"] >= 8 and 0.0 <= stats["cop_win_rate"] <= 1.0 and 1.0 <= stats["mean_episode_length"] <= 12.0
    assert {"mean_return/cop_0", "mean_return/cop_1", "mean_return/thief_0"} <= set(stats)
    # per slot: the 16 ticks of the call are the counted lengths plus the episode under way
    st = env.episode_tracker.per_slot()
    assert (st["len_sum"] + st["len_run"]).tolist() == [16] * 8
    stats = tr.train(8)                                     # cleared at the start of every call
    st = env.episode_tracker.per_slot()
    assert int(st["len_sum"].max()) <= 8 + 12


def test_self_play_with_tracked_evaluation_books_the_same_outcomes(tmp_path):
    """``win_rates.json`` with ``tracked_eval=True`` equals the one without, entry for entry, over several evaluations on the one
    evaluation env of a run, with episodes that end in captures and in timeouts on different ticks."""
    logs = {}
    for run, flag in (("base", False), ("tracked", True)):
        lines = logs.setdefault(run, [])
        kw = dict(training=TrainingConfig(n_trial_episodes=10, num_opponents_to_evaluate=2), trainer_cfg=TC, eval_envs=12,
                  role_cfg={"cop": RC, "thief": RC}, env_factory=TRACKED_LONG, iterations=3, log=lambda *a, lines=lines: lines.append(" ".join(map(str, a))))
        logs[run + " result"] = run_self_play("squarinth", 8, tmp_path / run, tracked_eval=flag, **kw)
    base, tracked = logs["base result"], logs["tracked result"]
    for d in ("cops", "thieves"):
        a, b = (json.loads((tmp_path / run / d / "win_rates.json").read_text()) for run in ("base", "tracked"))
        assert a == b and len(a) >= 1, d
    assert [h["evaluations"] for h in base["iterations"]] == [h["evaluations"] for h in tracked["iterations"]]
    assert base["param_digest"] == tracked["param_digest"]
    rates = [[tuple(float(v) for v in re.search(r"cop ([0-9.]+) thief ([0-9.]+)", line).groups()) for line in logs[run] if " vs " in line]
             for run in ("base", "tracked")]
    assert rates[0] == rates[1] and len(rates[0]) == 6      # 1 + 1 evaluations after iteration 1, 2 + 2 after iteration 2, all on one env
    assert sum(c > 0 and t > 0 for c, t in rates[0]) >= 2, rates[0]     # not a comparison of (0, 1) with (0, 1)
    with pytest.raises(TypeError):                          # envs without a tracker cannot serve the tracked evaluation
        run_self_play("squarinth", 8, tmp_path / "plain", tracked_eval=True, **dict(kw, env_factory=PLAIN))


def test_self_play_with_episode_stats(tmp_path):
    """With ``episode_stats=True`` the final parameters equal the ones without and ``episode_stats.json`` has one entry per iteration."""
    kw = dict(training=TrainingConfig(n_trial_episodes=3, num_opponents_to_evaluate=2), trainer_cfg=TC,
              role_cfg={"cop": RC, "thief": RC}, env_factory=TRACKED, log=lambda *a: None, iterations=3)
    base = run_self_play("squarinth", 8, tmp_path / "base", **kw)
    lines = []
    stats = run_self_play("squarinth", 8, tmp_path / "stats", episode_stats=True, **dict(kw, log=lambda *a: lines.append(" ".join(map(str, a)))))
    assert base["param_digest"] == stats["param_digest"]
    log = json.loads((tmp_path / "stats" / "episode_stats.json").read_text())
    assert [e["iteration"] for e in log] == [0, 1, 2]
    assert all(e["episodes"] >= 1 and 0.0 <= e["cop_win_rate"] <= 1.0 and e["mean_episode_length"] >= 1.0 and "mean_return/thief_0" in e for e in log)
    assert not (tmp_path / "base" / "episode_stats.json").exists()
    assert sum("cop win rate" in line for line in lines) == 3
