"""The geodesic start-state curriculum without a GPU: ``navigation.spawn_step`` (the definition) on hand-derived rows and against an
independent brute-force statement of the rule on the real maps, the fallback conditions read from the maps' own hop tables, the C ABI of
``cat_render_nav_spawn`` with its argument checks (which come before any device call), ``GeodesicSpawner`` on the oracle-backed stand-in env,
``adapt``'s rule on canned counters, every ValueError and the command line."""
import ctypes as C
import functools
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd import _learn_native as ln
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.navigation import NONE, NavField, separation, spawn_step
from as_cops_and_thieves_amd.selfplay import self_play as sp
from as_cops_and_thieves_amd.selfplay.curriculum import GeodesicSpawner, check_band
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
from tests import curriculum_cases as cc
from tests.curriculum_env import CurriculumOracleEnv
from tests.shaping_env import ShapingOracleEnv

ROOT = Path(__file__).resolve().parent.parent
t = torch.from_numpy
bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
PATTERN = -12345.0625            # the pre-fill of rows that must stay unwritten


def run_definition(mask, u, band, field, n_cops):
    """``spawn_step`` into pre-filled buffers: (positions float64 [N, A, 2], placed uint8 [N]) as NumPy arrays."""
    A, N = u.shape
    pos = torch.full((N, A, 2), PATTERN, dtype=torch.float64)
    placed = torch.full((N,), 7, dtype=torch.uint8)
    p, pl = spawn_step(t(mask), t(u), t(band), field, n_cops, positions=pos, placed=placed)
    assert p is pos and pl is placed
    return pos.numpy(), placed.numpy()


# ---------------------------------------------------------------------------------------------- 1. known answers
@pytest.mark.parametrize("rows,n_cops", [(cc.rows_2v1, 2), (cc.rows_1v2, 1)], ids=["2v1", "1v2"])
def test_spawn_step_gives_the_hand_derived_answers(rows, n_cops):
    rows = rows()
    b = cc.batch(rows, 3)
    pos, placed = run_definition(b["mask"], b["uniform"], b["band"], cc.make_field(b["slot_map"]), n_cops)
    for n, r in enumerate(rows):
        want = np.full((3, 2), PATTERN) if r["pos"] is cc.X else np.array(r["pos"], np.float64)
        assert placed[n] == (r["pos"] is not cc.X) and np.array_equal(bits64(pos[n]), bits64(want)), (r["name"], pos[n].tolist(), int(placed[n]))
    assert placed.sum() >= 2 and (n_cops == 1 or (placed == 0).sum() >= 6)


def test_the_special_draws_are_what_the_case_file_says():
    top, up = np.float32(cc.U_TOP), np.float32(cc.U_UP_9_OF_14)
    assert top.view(np.uint32) == 0x3F7FFFFF and all(int(top * np.float32(c)) == c - 1 for c in (1, 2, 3, 13, 14, 1296, 4096))
    assert float(up * np.float32(14)) == 9.0 and float(up) * 14 < 9.0          # (the f64 product is exact enough to show it)
    assert int(np.float32(1.0) * np.float32(14)) == 14                         # u = 1.0 is what the min clamps


def test_fresh_outputs_are_zero_where_nothing_is_placed_and_n_cops_is_checked():
    b = cc.batch(cc.rows_2v1(), 3)
    field = cc.make_field(b["slot_map"])
    pos, placed = spawn_step(t(b["mask"]), t(b["uniform"]), t(b["band"]), field, 2)
    assert pos.dtype == torch.float64 and placed.dtype == torch.uint8 and bool((pos[placed == 0] == 0).all())
    for bad in (0, 3, True, 1.0):
        with pytest.raises(ValueError):
            spawn_step(t(b["mask"]), t(b["uniform"]), t(b["band"]), field, bad)


# ---------------------------------------------------------------------------------------------- 2. the rule, brute force, on the real maps
@functools.lru_cache(maxsize=None)
def arena(name, n_cops, n_thieves, N):
    cm = load_preset(name, n_cops, n_thieves).compile()
    field = NavField.from_maps([cm], np.zeros(N, np.int32), 16, 6.0, "cpu", arena=True)
    return field, cc.tables_of(field)


N_BRUTE = 96


@pytest.mark.parametrize("name,roster", [("squarinth", (2, 1)), ("squarinth", (3, 2)), ("labyrinth", (2, 1))], ids=["squarinth-2v1", "squarinth-3v2", "labyrinth-2v1"])
def test_spawn_step_equals_an_independent_brute_force_of_the_rule(name, roster):
    n_cops, A = roster[0], sum(roster)
    field, tables = arena(name, *roster, N_BRUTE)
    free, hops, Hc = tables[0]
    mask, u, band, _ = cc.random_batch(11 + A, N_BRUTE, A, n_maps=1, hi_max=30)
    slot_map = np.zeros(N_BRUTE, np.int32)
    pos, placed = run_definition(mask, u, band, field, n_cops)
    cells, want_placed = cc.brute_force(mask, u, band, tables, slot_map, n_cops)
    assert np.array_equal(placed, want_placed) and 20 < placed.sum() < N_BRUTE
    want = cc.centres(cells, tables, slot_map)
    on = placed == 1
    assert np.array_equal(bits64(pos[on]), bits64(want[on]))                    # the centres, bit for bit
    assert np.array_equal(bits64(pos[~on]), bits64(np.full_like(pos[~on], PATTERN)))      # off, unmasked and fallback rows: the pre-fill stays
    # the properties, from the positions alone
    for n in np.flatnonzero(on):
        ix, iy = (pos[n, :, 0] / 16 - 0.5), (pos[n, :, 1] / 16 - 0.5)
        assert np.array_equal(ix, np.round(ix)) and np.array_equal(iy, np.round(iy))
        k = (ix * Hc + iy).astype(np.int64)
        assert len(set(k.tolist())) == A and free[k].all()
        thieves, cops = k[n_cops:], k[:n_cops]
        assert all(hops[thieves[0], b] != NONE for b in thieves[1:])
        for c in cops:
            d = min(int(hops[b, c]) for b in thieves if hops[b, c] != NONE)
            assert band[n, 0] <= d <= band[n, 1], (n, d, band[n])
    # ... and separation() of the f16 positions (what the env will show) says the same
    sep = separation(t(pos.astype(np.float32)).to(torch.float16), field, list(range(n_cops)), [sum(1 << j for j in range(n_cops, A))] * n_cops).numpy()
    assert ((sep[:, on] >= band[on, 0]) & (sep[:, on] <= band[on, 1])).all()


# ---------------------------------------------------------------------------------------------- 3. when the rule falls back
def candidates_per_anchor(tables, lo, hi):
    free, hops, _ = tables[0]
    idx = np.flatnonzero(free)
    sub = hops[np.ix_(idx, idx)]
    return ((sub >= lo) & (sub <= hi)).sum(axis=1)


def fallback_share(name, roster, band, N=512, seed=5):
    field, tables = arena(name, *roster, N)
    A = sum(roster)
    u = np.random.default_rng(seed).random((A, N), dtype=np.float32)
    pos, placed = run_definition(np.ones(N, np.uint8), u, np.tile(np.array(band, np.int32), (N, 1)), field, roster[0])
    assert np.array_equal(bits64(pos[placed == 0]), bits64(np.full_like(pos[placed == 0], PATTERN)))
    return 1.0 - placed.mean(), tables


def test_squarinth_never_falls_back_at_2_to_6_hops():
    """Squarinth's arena field: 1296 free cells, diameter 70; at band (2, 6) every anchor has at least 25 candidates, more than any roster
    here takes away, so the share of fallbacks is exactly 0."""
    for roster in ((2, 1), (3, 2)):
        share, tables = fallback_share("squarinth", roster, (2, 6))
        free, hops, _ = tables[0]
        assert free.sum() == 1296 and hops[hops != NONE].max() == 70 and candidates_per_anchor(tables, 2, 6).min() >= 25
        assert share == 0.0


def test_squarinth_falls_back_at_60_to_64_hops_and_leaves_those_rows_alone():
    """At band (60, 64) most anchors have no cell that far away (1032 of 1296 by this table): fallbacks must occur, each with ``placed == 0``
    and its positions unwritten (checked in ``fallback_share``) -- the env's own spawn stands."""
    share, tables = fallback_share("squarinth", (2, 1), (60, 64))
    none = int((candidates_per_anchor(tables, 60, 64) == 0).sum())
    assert none > 648                                # more than half of the anchors
    assert 0.5 < share < 1.0


def test_labyrinth_never_falls_back_at_2_to_6_hops():
    share, tables = fallback_share("labyrinth", (2, 1), (2, 6))
    assert candidates_per_anchor(tables, 2, 6).min() >= 12 and share == 0.0


# ---------------------------------------------------------------------------------------------- 4. the C ABI
def test_the_struct_matches_the_header():
    text = (ROOT / "include" / "cat_render.h").read_text()
    body = re.search(r"typedef struct cat_render_nav_spawn_args \{(.*?)\} cat_render_nav_spawn_args;", text, re.S).group(1)
    names = []
    for line in body.splitlines():
        decl = line.split("/*")[0].strip().rstrip(";")
        if decl:
            first, *more = [p.strip() for p in decl.split(",")]
            names += [re.sub(r"[\[\*].*", "", first.split()[-1].lstrip("*"))] + more
    assert names == [n for n, _ in ln.NavSpawnArgs._fields_]
    assert C.sizeof(ln.NavSpawnArgs) == 6 * 4 + 9 * 8
    assert "cat_render_nav_spawn" in ln.MODULES["cat_render"][1] and "cat_render_nav_spawn" in ln.RENDER_SYMBOLS


def test_bad_arguments_are_refused_before_any_device_call():
    """Every check of ``cat_render_nav_spawn`` comes before the launch, so a host without a GPU can ask for each refusal (the pointers are
    never followed)."""
    lib = ln.lib()
    keep = np.zeros(64, np.float64)
    ptr = keep.ctypes.data

    def args(**kw):
        base = dict(N=4, A=3, n_cops=2, n_maps=1, cell=16, pad=0, grid=ptr, free=ptr, hops=ptr, slot_map=ptr, mask=ptr, band=ptr, uniform=ptr,
                    positions=ptr, placed=ptr)
        base.update(kw)
        return ln.NavSpawnArgs(*[base[n] for n, _ in ln.NavSpawnArgs._fields_])

    def refused(what, **kw):
        rc = lib.cat_render_nav_spawn(C.byref(args(**kw)), None)
        msg = lib.cat_render_last_error().decode()
        assert rc != 0 and "cat_render_nav_spawn" in msg and what in msg, (kw, rc, msg)

    assert lib.cat_render_nav_spawn(None, None) != 0 and "NULL arguments" in lib.cat_render_last_error().decode()
    refused("bad dimensions", N=0)
    refused("bad dimensions", A=0)
    refused("CAT_RENDER_MAX_AGENTS", A=17, n_cops=2)
    for n_cops in (0, 3, -1):
        refused("n_cops", n_cops=n_cops)
    refused("n_maps", n_maps=0)
    refused("n_maps", n_maps=17)
    refused("cell", cell=0)
    for name in ("grid", "free", "hops"):
        refused("table of the field is NULL", **{name: None})
    for name in ("mask", "band", "uniform", "positions", "placed"):
        refused("required buffer is NULL", **{name: None})
    refused("8-byte aligned", positions=ptr + 4)


# ---------------------------------------------------------------------------------------------- 5. the spawner on the stand-in env
def make_env(cls=CurriculumOracleEnv, N=48, msc=8, seed=3):
    env = cls(load_preset("squarinth", 2, 1).compile(), N, num_rays=16, max_step_count=msc, seed=seed)
    env.reset()
    return env


def test_the_stand_in_env_respawns_terminal_slots_and_keeps_the_terminal_tick():
    """max_step_count 8, 20 random ticks.  Env A carries the spawner; env B has none and is driven by hand -- the same actions, then the
    oracle's ``reset(mask=placed, positions=positions)`` with A's outputs -- so B reports what "the same env without a spawner" reports
    for every tick.  After every terminal tick: the new episode's ``team_positions`` are the f16 of the chosen centres, ``step_count`` is
    0, and reward, flags and ``final_positions`` equal B's."""
    N = 48
    a, b = make_env(N=N), make_env(ShapingOracleEnv, N=N)
    spawner = GeodesicSpawner(a, 2, 6)
    assert not spawner.fused and spawner.band.tolist() == [[2, 6]] * N
    a.set_spawner(spawner)
    field, tables = arena("squarinth", 2, 1, N)
    gen = torch.Generator().manual_seed(4)
    terminal = 0
    for tick in range(20):
        acts = torch.randint(0, 4, (N, 3), generator=gen, dtype=torch.int32)
        ra, rb = a.step(acts), b.step(acts)
        term = ra[2]["cop_0"]
        assert torch.equal(term, rb[2]["cop_0"]) and torch.equal(ra[3]["cop_0"], rb[3]["cop_0"])
        assert all(torch.equal(ra[1][ag].view(torch.int32), rb[1][ag].view(torch.int32)) for ag in a.possible_agents)
        assert torch.equal(ra[4]["winner"], rb[4]["winner"])
        fa, fb = a.raw_outputs()["final_positions"], b.raw_outputs()["final_positions"]
        assert torch.equal(fa.view(torch.int16), fb.view(torch.int16))
        placed, pos = spawner.placed.clone(), spawner.positions.clone()
        assert torch.equal(placed.bool(), term)          # band (2, 6) on squarinth: no fallback
        b.sim.reset(mask=placed.numpy(), positions=pos.numpy())
        ta, tb = a.raw_outputs()["team_positions"], b.raw_outputs()["team_positions"]
        assert torch.equal(ta.view(torch.int16), tb.view(torch.int16))
        if bool(term.any()):
            terminal += int(term.sum())
            assert torch.equal(ta[term], pos[term].to(torch.float16)) and torch.equal(ta[term].double(), pos[term])     # exact in f16
            assert (a.sim.get_state()["step_count"][term.numpy()] == 0).all()
            d = separation(ta, field, [0, 1], [0b100, 0b100])[:, term]
            assert bool(((d >= 2) & (d <= 6)).all())
    assert terminal >= 2 * N
    c = spawner.counters()
    assert c["ended"] == terminal == c["requested"] == c["placed_total"] and 0 <= c["cop_wins"] <= terminal


def test_reset_places_the_slots_and_off_slots_keep_the_maps_spawn():
    N = 32
    a, b = make_env(N=N), make_env(N=N)
    spawner = GeodesicSpawner(a, 3, 5, slots=slice(0, 20))
    assert spawner.band[:20].tolist() == [[3, 5]] * 20 and spawner.band[20:].tolist() == [[-1, -1]] * 12
    a.set_spawner(spawner)
    a.reset(); b.reset()
    ta, tb = a.raw_outputs()["team_positions"], b.raw_outputs()["team_positions"]
    assert spawner.reset_placed.tolist() == [1] * 20 + [0] * 12
    assert torch.equal(ta[20:].view(torch.int16), tb[20:].view(torch.int16))     # off: the map's own spawn, the same Philox draw
    field, _ = arena("squarinth", 2, 1, N)
    d = separation(ta, field, [0, 1], [0b100, 0b100])[:, :20]
    assert bool(((d >= 3) & (d <= 5)).all())
    spawner.set_off(slice(0, 10))
    spawner.set_band(4, 4, slots=torch.arange(10, 20))
    assert spawner.band[:10].tolist() == [[-1, -1]] * 10 and spawner.band[10:20].tolist() == [[4, 4]] * 10 and (spawner.lo, spawner.hi) == (4, 4)


# ---------------------------------------------------------------------------------------------- 6. adapt, and everything that raises
def canned(spawner, ended, wins):
    spawner.ended.fill_(ended); spawner.cop_wins.fill_(wins)


def test_adapt_moves_hi_with_the_win_rate_and_clears_the_counters():
    env = make_env(N=8)
    s = GeodesicSpawner(env, 2, 6, slots=slice(0, 6))
    assert s.adapt(0.3, 0.7) == 6 and s.last["ended"] == 0                      # nothing ended: no change
    canned(s, 10, 8)
    assert s.adapt(0.3, 0.7) == 7 and s.band[:6, 1].tolist() == [7] * 6 and s.band[6:].tolist() == [[-1, -1]] * 2
    assert s.counters() == dict(ended=0, cop_wins=0, requested=0, placed_total=0) and s.last["cop_wins"] == 8
    canned(s, 10, 7)                                                            # w == high: not above it
    assert s.adapt(0.3, 0.7) == 7
    canned(s, 10, 3)                                                            # w == low: not below it
    assert s.adapt(0.3, 0.7) == 7
    canned(s, 10, 2)
    assert s.adapt(0.3, 0.7, step=3) == 4
    canned(s, 10, 0)
    assert s.adapt(0.3, 0.7, step=3) == 2                                       # down to lo
    canned(s, 10, 0)
    assert s.adapt(0.3, 0.7) == 2
    canned(s, 10, 10)
    assert s.adapt(0.3, 0.7, step=5, hi_max=6) == 6                             # up to hi_max
    canned(s, 10, 0)
    assert s.adapt(0.3, 0.7, step=5, hi_min=4) == 4                             # down to max(lo, hi_min)
    assert s.band[:, 0].tolist() == [2] * 6 + [-1] * 2
    for kw in (dict(step=0), dict(step=1.5), dict(low=0.8, high=0.2), dict(high=1.5)):
        with pytest.raises(ValueError):
            s.adapt(**dict(dict(low=0.3, high=0.7), **kw))


@pytest.mark.parametrize("band", [(0, 3), (3, 2), (1, 65535), (-1, -1), (1.0, 2), (True, 2), (1, None)])
def test_set_band_refuses_everything_but_a_band(band):
    with pytest.raises(ValueError):
        check_band(*band)
    s = GeodesicSpawner(make_env(N=4), 1, 65534)
    with pytest.raises(ValueError):
        s.set_band(*band)
    assert s.band.tolist() == [[1, 65534]] * 4
    with pytest.raises(ValueError):
        GeodesicSpawner(make_env(N=4), *band)


@pytest.mark.parametrize("kw", [dict(spawn_curriculum=(0, 3)), dict(spawn_curriculum=(4, 3)), dict(spawn_curriculum=(1, 65535)), dict(spawn_curriculum=(1.5, 3)),
                                dict(spawn_curriculum=3), dict(curriculum_fraction=1.5), dict(curriculum_fraction=-0.1), dict(curriculum_fraction=float("nan")),
                                dict(curriculum_adapt=(0.2, 0.8)), dict(spawn_curriculum=(2, 6), curriculum_adapt=(0.8, 0.2)),
                                dict(spawn_curriculum=(2, 6), curriculum_adapt=(0.2, 1.2)), dict(curriculum_step=0), dict(curriculum_step=1.5),
                                dict(curriculum_max=0), dict(curriculum_max=65535), dict(spawn_curriculum=(2, 70), curriculum_max=64)])
def test_trainer_config_refuses_bad_curriculum_fields(kw):
    with pytest.raises(ValueError):
        TrainerConfig(**kw)


def test_trainer_config_defaults_are_off():
    tc = TrainerConfig()
    assert tc.spawn_curriculum is None and tc.curriculum_adapt is None and (tc.curriculum_fraction, tc.curriculum_step, tc.curriculum_max) == (1.0, 1, 64)
    assert TrainerConfig(spawn_curriculum=[2, 6], curriculum_adapt=[0.25, 0.75]).spawn_curriculum == (2, 6)


def test_rollout_random_with_a_spawner_raises():
    env = make_env(N=4)
    env.set_spawner(GeodesicSpawner(env, 2, 6))
    with pytest.raises(ValueError, match="spawner"):
        env.rollout_random(4)
    src = (ROOT / "as_cops_and_thieves_amd" / "environments.py").read_text()     # VecCopsEnv's own refusal comes before any launch
    body = src[src.index("def rollout_random"):src.index("def _tracked_keys")]
    assert body.index("self._spawner is not None") < body.index("self._sim.rollout_fused")


def test_the_trainer_attaches_a_spawner_and_reports_and_saves_it():
    env = make_env(N=8, msc=6)
    rc = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0)
    tc = TrainerConfig(horizon=8, bptt=8, timesteps=16, policy_freeze_duration=0, opponent_freeze_duration=0, spawn_curriculum=(2, 6),
                       curriculum_fraction=0.5, curriculum_adapt=(0.3, 0.7), curriculum_max=9)
    tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, tc, seed=1)
    assert env._spawner is tr._spawner and tr._spawner.band[:, 0].tolist() == [2] * 4 + [-1] * 4
    assert tr._random_phase_span(0, 1 << 20) == 0
    with torch.enable_grad():
        stats = tr.train(16)
    assert {"curriculum/hi", "curriculum/cop_win_rate", "curriculum/placed", "curriculum/fallbacks"} <= set(stats)
    assert stats["curriculum/fallbacks"] == 0 and stats["curriculum/placed"] > 0 and 2 <= stats["curriculum/hi"] <= 9
    sd = tr.state_dict()
    assert sd[tr.META_KEY]["curriculum"] == {"lo": 2, "hi": tr._spawner.hi}
    # a trainer without the option: no spawner, the same checkpoint loads with one warning; and the other way round the band is restored
    env2 = make_env(N=8, msc=6)
    plain = MAPPOTrainer(env2, {"cop": rc, "thief": rc}, TrainerConfig(horizon=8, bptt=8, policy_freeze_duration=0, opponent_freeze_duration=0), seed=1)
    assert plain._spawner is None and env2._spawner is None and "curriculum" not in plain.state_dict()[plain.META_KEY]
    with pytest.warns(UserWarning, match="start-state curriculum"):
        plain.load_state_dict(sd)
    sd[tr.META_KEY]["curriculum"] = {"lo": 3, "hi": 8}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr.load_state_dict(sd)
    assert tr._spawner.band[:4].tolist() == [[3, 8]] * 4 and tr._spawner.band[4:].tolist() == [[-1, -1]] * 4
    del sd[tr.META_KEY]["curriculum"]                     # a checkpoint without it: the band stays
    tr.load_state_dict(sd)
    assert tr._spawner.band[:4].tolist() == [[3, 8]] * 4


# ---------------------------------------------------------------------------------------------- 7. the command line
def test_the_command_line_parses_the_curriculum_options():
    ap = sp.build_parser()
    off = ap.parse_args([])
    assert sp.curriculum_options(off) == {}
    args = ap.parse_args("--spawn-curriculum 2 6 --curriculum-fraction 0.5 --curriculum-adapt 0.3 0.7 --curriculum-step 2 --curriculum-max 40 "
                         "--separation-eval 2:6,10:14,30:34 --separation-episodes 16".split())
    assert sp.curriculum_options(args) == dict(spawn_curriculum=(2, 6), curriculum_fraction=0.5, curriculum_adapt=(0.3, 0.7), curriculum_step=2,
                                               curriculum_max=40, separation_eval=[(2, 6), (10, 14), (30, 34)], separation_episodes=16)
    assert sp.curriculum_options(ap.parse_args(["--spawn-curriculum", "3", "3"])) == dict(spawn_curriculum=(3, 3), curriculum_fraction=1.0,
                                                                                         curriculum_step=1, curriculum_max=64)
    for text in ("2-6", "2:6;3:4", "6:2", "0:3", "a:b", "2:6,"):
        with pytest.raises(ValueError):
            sp.parse_separation_bands(text)
    with pytest.raises(SystemExit):
        ap.parse_args(["--spawn-curriculum", "2"])


@pytest.mark.parametrize("argv", [["--spawn-curriculum", "2", "6", "--gpus", "2"], ["--separation-eval", "2:6", "--gpus", "2"],
                                  ["--curriculum-adapt", "0.3", "0.7"]])
def test_the_command_line_refuses_what_cannot_apply(argv):
    with pytest.raises(ValueError):
        sp.main(argv)                                     # raised before anything is started or built
