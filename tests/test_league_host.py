"""CPU: the league form of the act tick -- ``cat_act_league_args`` in include/cat_act.h against the library and its ctypes mirror, the
entry's argument checks (no device needed), the unfused ``LeagueActor`` on the oracle-backed stand-in env against plain stacked
policies holding the same sets, and the self-play loop with ``league_eval``."""
import ctypes as C
import json
import re
import warnings
from pathlib import Path

import pytest
import torch

from as_cops_and_thieves_amd import _learn_native as ln
from as_cops_and_thieves_amd import packing
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.selfplay.actor import LeagueActor, PolicyActor, first_max_index
from as_cops_and_thieves_amd.selfplay.mappo import RoleConfig, TrainerConfig
from as_cops_and_thieves_amd.selfplay.self_play import TrainingConfig, evaluate_league, run_self_play
from tests.fake_env import OracleVecEnv

warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")
ROOT = Path(__file__).resolve().parents[1]
CMAP = load_preset("squarinth", 2, 1).compile()
RC = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=4, learning_starts=8, kl_threshold=0.0)
TC = TrainerConfig(horizon=4, timesteps=16, policy_freeze_duration=8, opponent_freeze_duration=8)
AGENTS = ["cop_0", "cop_1", "thief_0"]


# ---------------------------------------------------------------------------------------------- 1. header, library, mirror
def test_league_header_matches_the_library_and_the_ctypes_mirror():
    from tests.test_abi_and_isolation import test_learner_kernel_headers_match_the_library_and_the_ctypes_mirror as header_check
    header_check("cat_act.h", "cat_act_", "ACT_SYMBOLS", {"cat_act_dims": "ActDims", "cat_act_params": "ActParams", "cat_act_args": "ActArgs",
                                                         "cat_act_league_args": "ActLeagueArgs"})
    assert ln.ACT_SYMBOLS[-1] == "cat_act_league_step" and hasattr(ln.lib(), "cat_act_league_step")
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_act.h").read_text(), flags=re.S)
    assert int(re.search(r"#define CAT_ACT_MAX_SEGMENTS (\d+)", code).group(1)) == ln.ACT_MAX_SEGMENTS == 32
    assert int(re.search(r"#define CAT_ACT_ABI_VERSION (\d+)", code).group(1)) == 1 == ln.lib().cat_act_abi_version()
    # cat_act_args (280 bytes, pinned by tests/test_actor_host.py), S, sets, seg_start[33], seg_set[8][32]: 1444 bytes, 8-aligned -> 1448
    assert C.sizeof(ln.ActArgs) == 280
    assert C.sizeof(ln.ActLeagueArgs) == 1448 == (280 + 2 * 4 + 33 * 4 + 8 * 32 * 4 + 7) // 8 * 8 < 4096
    assert (ln.ActLeagueArgs.base.offset, ln.ActLeagueArgs.S.offset, ln.ActLeagueArgs.sets.offset) == (0, 280, 284)
    assert (ln.ActLeagueArgs.seg_start.offset, ln.ActLeagueArgs.seg_set.offset) == (288, 288 + 33 * 4)


def _league_args(N=10, S=2, sets=2, start=(0, 4, 10), dims=None):
    a = ln.ActLeagueArgs()
    a.base.d = ln.ActDims(*(dims or (3, N, 3, 64)))
    for g in range(3):
        a.base.agent[g] = g
    a.S, a.sets = S, sets
    for s, v in enumerate(start):
        a.seg_start[s] = v
    return a


def test_league_entry_rejects_bad_arguments_before_touching_a_device():
    L = ln.lib()

    def rejected(a, word):
        rc, msg = L.cat_act_league_step(C.byref(a), None), L.cat_act_last_error()
        assert rc == -1 and word in msg and msg.startswith(b"cat_act_league_step"), (rc, msg, word)

    # a well-formed table reaches the buffer checks (and stops there: every pointer is NULL)
    rejected(_league_args(), b"NULL")
    assert L.cat_act_league_step(None, None) == -1
    for S in (0, -1, 33):
        rejected(_league_args(S=S), b"S outside")
    for sets in (0, -3):
        rejected(_league_args(sets=sets), b"parameter set")
    rejected(_league_args(start=(1, 4, 10)), b"begin at 0")
    rejected(_league_args(start=(0, 4, 9)), b"end at N")
    rejected(_league_args(start=(0, 4, 11)), b"end at N")
    rejected(_league_args(start=(0, 0, 10)), b"strictly increasing")
    rejected(_league_args(S=3, start=(0, 6, 4, 10)), b"strictly increasing")
    for bad in (2, -2, 100):
        a = _league_args()
        a.seg_set[2][1] = bad
        rejected(a, b"set index")
    a = _league_args()
    a.seg_set[1][0] = -1                                         # -1 itself is the random policy: accepted
    rejected(a, b"NULL")
    a = _league_args()
    a.seg_set[5][1] = 7                                          # rows of policies beyond G are not read
    rejected(a, b"NULL")
    a = _league_args()
    a.base.random_mask = 1
    rejected(a, b"random_mask")
    for dims in ((3, 10, 3, 72), (9, 10, 3, 64), (0, 10, 3, 64), (3, 0, 3, 64), (3, 10, 9, 64)):
        assert L.cat_act_supported(C.byref(ln.ActDims(*dims))) == 0
        rejected(_league_args(dims=dims), b"dimensions")
    # the plain entry keeps its messages
    assert L.cat_act_step(C.byref(ln.ActArgs()), None) == -1 and L.cat_act_last_error().startswith(b"cat_act_step: bad dimensions")


def test_league_table_applies_the_entrys_rules_in_python():
    t = ln.league_table(10, 3, 2, [0, 4, 10], [[0, 1], [1, -1], [0, 0]])
    assert (t.S, list(t.seg_start[:3]), [list(r[:2]) for r in t.seg_set[:3]]) == (2, [0, 4, 10], [[0, 1], [1, -1], [0, 0]])
    for start, table in (([0, 10], [[0], [0]]), ([1, 10], [[0]] * 3), ([0, 9], [[0]] * 3), ([0, 4, 4, 10], [[0] * 3] * 3), ([0, 10], [[2]] * 3),
                         ([0, 10], [[-2]] * 3), (list(range(34)), [[0] * 33] * 3), ([0], [[]] * 3)):
        with pytest.raises(ValueError):
            ln.league_table(start[-1] if start[-1] == 33 else 10, 3, 2, start, table)
    with pytest.raises(ValueError):
        ln.league_table(10, 3, 0, [0, 10], [[0]] * 3)


# ---------------------------------------------------------------------------------------------- 2. the unfused LeagueActor
SEGMENTS = [(0, 1, {"cop_0": 0, "cop_1": 0, "thief_0": 1}),            # one set serves two agents
            (1, 4, {"cop_0": 2, "cop_1": "random", "thief_0": 0}),
            (4, 7, {"cop_0": 1, "cop_1": 2, "thief_0": 2})]


@pytest.fixture(scope="module")
def league():
    """The league actor after ONE greedy tick from a random state, and everything the checks need of before and after."""
    env = OracleVecEnv(CMAP, 7, num_rays=16, max_step_count=12, seed=3)
    assert env.possible_agents == AGENTS
    actor = LeagueActor.from_env(env, 3, fused=False, seed=4)
    assert not actor.fused and actor.sets == 3 and actor.N == 7 and actor.agents == AGENTS and actor.actions.shape == (7, 3)
    name = "policy.policy_head.0.weight"
    assert not torch.equal(actor.bank.views[name][0], actor.bank.views[name][1]) and not torch.equal(actor.bank.views[name][1], actor.bank.views[name][2])
    actor.set_matchups(SEGMENTS)
    assert actor.segments == [(0, 1), (1, 4), (4, 7)]
    obs, _ = env.reset()
    gen = torch.Generator().manual_seed(11)
    (key,) = actor.state
    before = {key: tuple(torch.randn(t.shape, generator=gen) * 0.5 for t in actor.state[key])}
    actor.set_state(before)
    starts = torch.tensor([False, True, False, False, False, True, False])
    logits = torch.full((3, 7, 4), float("nan"))
    actions = actor.act(env, starts, greedy=True, obs=obs, logits_out=logits).clone()
    # the plain stacked policies: actor k holds set k in every row
    plain = []
    for k in range(3):
        p = PolicyActor.from_checkpoint(None, env, fused=False, seed=99)
        (grp,) = p.groups.values()
        grp.fp.lp.copy_(actor.bank.lp[k].expand_as(grp.fp.lp))
        plain.append(grp)
    pin = torch.stack([packing.pack_policy_input(obs[a]) for a in AGENTS])
    return {"actor": actor, "env": env, "obs": obs, "before": before[key], "after": tuple(t.clone() for t in actor.state[key]), "starts": starts,
            "logits": logits, "actions": actions, "plain": plain, "pin": pin}


@pytest.mark.parametrize("s", range(3))
@pytest.mark.parametrize("g", range(3))
def test_every_agent_and_segment_equals_the_plain_stacked_policy_holding_its_set(league, g, s):
    lo, hi, who = SEGMENTS[s]
    k = who[AGENTS[g]]
    h0, c0 = league["before"]
    h1, c1 = league["after"]
    if k == "random":
        assert torch.equal(h1[:, g, lo:hi], h0[:, g, lo:hi]) and torch.equal(c1[:, g, lo:hi], c0[:, g, lo:hi])      # state rows untouched
        assert bool(torch.isnan(league["logits"][g, lo:hi]).all())
        assert bool(((league["actions"][lo:hi, g] >= 0) & (league["actions"][lo:hi, g] <= 3)).all())
        return
    keep = (~league["starts"][lo:hi]).view(1, hi - lo)
    with torch.no_grad():
        z, (h, c) = league["plain"][k].policy.forward(league["pin"][:, lo:hi].unsqueeze(1), (h0[:, :, lo:hi], c0[:, :, lo:hi]), keep)
    assert torch.equal(league["logits"][g, lo:hi], z[g, 0].float())
    assert torch.equal(h1[:, g, lo:hi], h[:, g]) and torch.equal(c1[:, g, lo:hi], c[:, g])
    assert not torch.equal(h1[:, g, lo:hi], h0[:, g, lo:hi])
    assert torch.equal(league["actions"][lo:hi, g].long(), first_max_index(z[g, 0].float()))


def test_random_cells_draw_all_four_actions_and_sampled_ticks_follow_the_generator(league):
    actor, env, obs = league["actor"], league["env"], league["obs"]
    seen = set()
    for _ in range(40):
        seen |= set(actor.act(env, greedy=True, obs=obs)[1:4, 1].tolist())
    assert seen == {0, 1, 2, 3}
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        actor.reset()
        runs.append(torch.stack([actor.act(env, obs=obs).clone() for _ in range(3)]))
    assert torch.equal(*runs) and bool(((runs[0] >= 0) & (runs[0] <= 3)).all())
    with pytest.raises(ValueError):
        actor.act(env, random_roles=("thief",), obs=obs)
    with pytest.raises(TypeError):
        actor.load({})


def test_load_set_reads_both_checkpoint_layouts(tmp_path):
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer
    env = OracleVecEnv(CMAP, 4, num_rays=16, max_step_count=12, seed=1)
    runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, TC, seed=7)
    sd = runner.state_dict()
    torch.save(sd, tmp_path / "cat.pt")
    del sd[MAPPOTrainer.META_KEY]                                # what skrl's MAPPO.save writes
    torch.save(sd, tmp_path / "reference.pt")
    actor = LeagueActor.from_env(env, 2, fused=False)
    actor.load_set(0, tmp_path / "cat.pt", "thief_0")
    actor.load_set(1, tmp_path / "reference.pt", "cop_1")
    for k, a in ((0, "thief_0"), (1, "cop_1")):
        rl, gr = runner.learner_of(a)
        for n in actor.bank.names:
            assert torch.equal(actor.bank.views[n][k], rl.fp.views[n][gr].detach()), (a, n)
    with pytest.raises(KeyError):
        actor.load_set(0, tmp_path / "cat.pt", "thief_7")
    with pytest.raises(IndexError):
        actor.load_set(2, tmp_path / "cat.pt", "cop_0")


def test_set_matchups_raises_on_each_malformed_table():
    env = OracleVecEnv(CMAP, 7, num_rays=16, max_step_count=12, seed=3)
    actor = LeagueActor.from_env(env, 3, fused=False)
    with pytest.raises(RuntimeError):
        actor.act(env)
    ok = {"cop_0": 0, "cop_1": 1, "thief_0": 2}
    actor.set_matchups([(0, 7, ok)])
    bad = {"a gap": [(0, 3, ok), (4, 7, ok)], "an overlap": [(0, 4, ok), (3, 7, ok)], "not from 0": [(1, 7, ok)], "not to N": [(0, 6, ok)],
           "beyond N": [(0, 8, ok)], "an empty segment": [(0, 3, ok), (3, 3, ok), (3, 7, ok)], "no segments": [],
           "a set beyond the bank": [(0, 7, dict(ok, cop_0=3))], "a negative set": [(0, 7, dict(ok, cop_0=-1))],
           "an agent missing": [(0, 7, {"cop_0": 0, "cop_1": 1})], "an unknown agent": [(0, 7, dict(ok, thief_1=0))],
           "an unknown word": [(0, 7, dict(ok, thief_0="greedy"))], "a float": [(0, 7, dict(ok, thief_0=1.0))]}
    for what, table in bad.items():
        with pytest.raises(ValueError):
            actor.set_matchups(table)
            pytest.fail(what)
    assert actor.segments == [(0, 7)]                            # a refused table leaves the current one in place


def test_evaluate_league_counts_the_first_episode_of_every_counted_slot():
    env = OracleVecEnv(CMAP, 7, num_rays=16, max_step_count=12, seed=3)
    actor = LeagueActor.from_env(env, 3, fused=False, seed=4)
    actor.set_matchups(SEGMENTS)
    torch.manual_seed(2)
    res = evaluate_league(env, actor, [1, 2, 0])
    assert res["episodes"] == [1, 2, 0]
    assert [c + t + o for c, t, o in zip(res["cop_wins"], res["thief_wins"], res["timeouts"])] == [1, 2, 0]
    assert res["winner"].tolist()[3:] == [-1] * 4 and all(w in (0, 1) for w in res["winner"].tolist()[:3])
    assert all(1 <= n <= 12 for n in res["length"].tolist()[:3]) and res["length"].tolist()[3:] == [0] * 4 and 1 <= res["ticks"] <= 12


# ---------------------------------------------------------------------------------------------- 3. self-play with league_eval
def test_self_play_with_league_eval_books_the_same_opponents(tmp_path):
    factory = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=12, seed=s)
    runs = {}
    for league_eval in (False, True):
        out = tmp_path / str(league_eval)
        lines = []
        res = run_self_play("squarinth", 8, out, iterations=3, training=TrainingConfig(n_trial_episodes=3, num_opponents_to_evaluate=2),
                            trainer_cfg=TC, role_cfg={"cop": RC, "thief": RC}, env_factory=factory, seed=0, league_eval=league_eval,
                            log=lambda *a: lines.append(" ".join(map(str, a))))
        rates = {d: json.loads((out / d / "win_rates.json").read_text()) for d in ("cops", "thieves")}
        runs[league_eval] = (res, rates, lines)
    for it in range(3):                                          # the archives hold `it` <= 2 files: every one of them is drawn either way
        a, b = (runs[k][0]["iterations"][it]["evaluations"] for k in (False, True))
        assert {r: set(v) for r, v in a.items()} == {r: set(v) for r, v in b.items()}, it
        assert all(len(b[r]) == min(it, 2) for r in ("cop", "thief"))
    for d, role in (("cops", "cop"), ("thieves", "thief")):
        a, b = runs[False][1][d], runs[True][1][d]
        assert set(a) == set(b) == {f"{role}_iter_0.pt", f"{role}_iter_1.pt"}
        assert {n: v["games"] for n, v in a.items()} == {n: v["games"] for n, v in b.items()} == {f"{role}_iter_0.pt": 2, f"{role}_iter_1.pt": 1}
        assert all(set(v) == {"wins", "games", "recent_outcomes", "buffer_size"} and len(v["recent_outcomes"]) == v["games"] for v in b.values())
    shape = lambda lines: sorted(re.sub(r"\d\.\d\d|won|lost", "#", line) for line in lines if " vs " in line)
    assert shape(runs[False][2]) == shape(runs[True][2]) and len(shape(runs[True][2])) == 6
    with pytest.raises(ValueError):
        run_self_play("squarinth", 8, tmp_path / "both", iterations=1, env_factory=factory, league_eval=True, tracked_eval=True, log=lambda *a: None)


# ---------------------------------------------------------------------------------------------- the cross-play table on the stand-in env
def test_crossplay_fills_every_cell_over_more_than_one_pass(tmp_path):
    from as_cops_and_thieves_amd.selfplay.crossplay import crossplay
    from as_cops_and_thieves_amd.selfplay.stacked import agent_state_dict
    factory = lambda n, s: OracleVecEnv(CMAP, n, num_rays=16, max_step_count=12, seed=s)
    env = factory(2, 0)
    for role, d, seeds in (("cop", "cops", range(7)), ("thief", "thieves", range(7, 11))):
        (tmp_path / d).mkdir()
        for it, seed in enumerate(seeds):
            (grp,) = PolicyActor.from_checkpoint(None, env, fused=False, seed=seed).groups.values()
            torch.save({a: {"policy": agent_state_dict(grp.fp, g)["policy"]} for g, a in enumerate(grp.agents)}, tmp_path / d / f"{role}_iter_{it}.pt")
    seen = []
    table = crossplay(tmp_path / "cops", tmp_path / "thieves", "squarinth", 2, random_column=True, fused=False, env_factory=factory, seed=4,
                      log=seen.append)
    assert table["cops"] == [f"cop_iter_{i}.pt" for i in range(7)] and table["thieves"] == [f"thief_iter_{i}.pt" for i in range(4)] + ["random"]
    assert table["passes"] == 2 == len(seen) and "32 cells" in seen[0] and "3 cells" in seen[1]            # 35 cells, at most 32 per pass
    for k in ("cop_win_rate", "cop_wins", "thief_wins", "timeouts", "mean_length"):
        assert len(table[k]) == 7 and all(len(row) == 5 for row in table[k]), k
    for i in range(7):
        for j in range(5):
            assert table["cop_wins"][i][j] + table["thief_wins"][i][j] + table["timeouts"][i][j] == 2
            assert table["cop_win_rate"][i][j] == table["cop_wins"][i][j] / 2 and 1 <= table["mean_length"][i][j] <= 12
    with pytest.raises(ValueError):
        crossplay(tmp_path / "cops", tmp_path / "nothing", "squarinth", 2, fused=False, env_factory=factory)
