"""Position statistics without a GPU: the NumPy form of the counting rule (positions.PositionTracker on CPU tensors) against a plain
per-row loop, its invariants, the C ABI of cat_render_positions_update and its argument checks (which come before any device call),
the heatmap colouriser, and the env hook on the oracle-backed stand-in env."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd.maps import PLANE_STRIDE, CompiledMap, load_preset
from as_cops_and_thieves_amd.positions import OCC, SEEN, SPAWN, PositionTracker, grid_shape
from as_cops_and_thieves_amd.render import HEAT_PALETTE, render_heatmap, write_heatmaps
from tests.fake_env import OracleVecEnv
from tests.positions_cases import loop_reference, synthetic_stream

ROOT = Path(__file__).resolve().parents[1]
NAN, INF = float("nan"), float("inf")


def _tracker(N, A, n_cops, W, H, cell, G=1):
    return PositionTracker(N, [f"a{i}" for i in range(A)], n_cops, (W, H), cell, G)


def _feed(tr, pos, term, obs, one_by_one=False):
    p, t = torch.from_numpy(pos), torch.from_numpy(term)
    o = None if obs is None else torch.from_numpy(obs)
    if one_by_one:
        for k in range(pos.shape[0]):
            tr.update(p[k], t[k], None if o is None else o[k])
    else:
        tr.update(p, t, o)


def _assert_equal(got, want, ctx=""):
    for k in ("counts", "outside", "rows", "done"):
        assert np.array_equal(got[k], want[k]), (ctx, k)


# ---------------------------------------------------------------------------------------------- 1. the CPU form against a loop
def _hand_built():
    """4 slots x 2 agents (1 cop, 1 thief), window 40 x 30, cell 8 (5 x 4 cells), 3 rays, 6 rows."""
    T, N, A, R = 6, 4, 2, 3
    pos = np.zeros((T, N, A, 2), np.float16)
    term = np.zeros((T, N), np.uint8)
    obs = np.full((T, N, A, R), 4, np.uint8)
    # slot 0 (group 0): the cop crosses from cell (0, 0) to (1, 0) and then stands on x == W exactly; the thief stays in cell (4, 3)
    for t, x in enumerate((7.0, 7.5, 8.0, 9.0, 40.0, 39.5)):
        pos[t, 0, 0] = (x, 3.0)
        pos[t, 0, 1] = (39.0, 29.0)
    term[3, 0] = 1                                   # a terminal row: a spawn for both agents
    obs[0, 0, 1, 2] = 1                              # row 0: the thief sees a cop -> the cop is seen
    obs[1, 0, 0, 0] = 2                              # row 1: the cop sees a thief -> the thief is seen
    obs[2, 0, 0, 1] = 1                              # row 2: the cop sees a COP: nobody of the other role sees anything
    obs[3, 0, 1, 0] = 1                              # the terminal row: no SEEN on a spawn
    # slot 1 (group 1): NaN, inf, a negative coordinate and a position outside the grid, then two good rows
    for t, xy in enumerate(((NAN, 3.0), (5.0, INF), (-0.5, 3.0), (100.0, 5.0), (5.0, 5.0), (5.0, 31.9))):
        pos[t, 1, 0] = xy
        pos[t, 1, 1] = (12.0, 12.0)
    # slot 2: group -1, never counted
    pos[:, 2] = 20.0
    term[2, 2] = 1
    # slot 3 (group 0) with a quota of 1: its first terminal row is row 2, rows 3.. are skipped
    pos[:, 3, 0] = (17.0, 9.0)
    pos[:, 3, 1] = (25.0, 17.0)
    term[2, 3] = term[4, 3] = 1
    obs[:, 3, 0, 1] = 2
    group = np.array([0, 1, -1, 0], np.int32)
    quota = np.array([5, 5, 5, 1], np.int32)
    return pos, term, obs, group, quota


def test_the_cpu_form_equals_the_loop_on_hand_built_rows():
    pos, term, obs, group, quota = _hand_built()
    tr = _tracker(4, 2, 1, 40, 30, 8, G=2)
    assert (tr.Wc, tr.Hc) == (5, 4) == grid_shape((40, 30), 8)
    tr.set_groups(group)
    tr.set_quota(quota)
    _feed(tr, pos, term, obs)
    got = tr.counts()
    _assert_equal(got, loop_reference(pos, term, obs, group, quota, 1, 8, 5, 4, 2))
    c = got["counts"]
    # the figures, by hand.  group 0 = slot 0 (6 rows) + slot 3 (3 rows: 0, 1 and the terminal row 2)
    assert got["rows"].tolist() == [9, 6] and got["done"].tolist() == [1, 0, 0, 1]
    assert c[0, OCC, 0, 0, 0] == 2 and c[0, OCC, 0, 1, 0] == 1 and c[0, OCC, 0, 4, 0] == 1     # cop of slot 0: 7.0, 7.5 | 8.0 | 39.5
    assert c[0, SPAWN, 0, 1, 0] == 1 and got["outside"][0, 0] == 1                           # 9.0 on the terminal row; x == W is outside
    assert c[0, OCC, 1, 4, 3] == 5 and c[0, SPAWN, 1, 4, 3] == 1
    assert c[0, SEEN, 0, 0, 0] == 1 and c[0, SEEN, 0].sum() == 1                              # row 0 only
    assert c[0, SEEN, 1, 4, 3] == 1                                                           # row 1 only (slot 0's thief)
    assert c[0, OCC, 0, 2, 1] == 2 and c[0, SPAWN, 0, 2, 1] == 1 and c[0, SEEN, 0, 2, 1] == 0  # slot 3's cop: nobody sees a cop
    assert c[0, OCC, 1, 3, 2] == 2 and c[0, SEEN, 1, 3, 2] == 2 and c[0, SPAWN, 1, 3, 2] == 1  # slot 3's thief is seen on both rows
    assert got["outside"][1].tolist() == [4, 0] and c[1, OCC, 0, 0, 0] == 1 and c[1, OCC, 0, 0, 3] == 1 and c[1, OCC, 1, 1, 1] == 6
    assert c[1, SEEN].sum() == 0 and c[:, :, :, 2, 2].sum() == 0                              # slot 2 (20, 20) was never counted
    # without obs_type: the same maps with an empty SEEN plane
    tr2 = _tracker(4, 2, 1, 40, 30, 8, G=2)
    tr2.set_groups(group)
    tr2.set_quota(quota)
    _feed(tr2, pos, term, None)
    want = {k: v.copy() for k, v in got.items()}
    want["counts"][:, SEEN] = 0
    _assert_equal(tr2.counts(), want)
    # the summary is formed from the counts
    s = tr.summary()
    assert s[0]["rows"] == 9 and s[0]["agents"]["a0"]["outside"] == 1 and s[0]["agents"]["a0"]["cells_visited"] == 4
    assert s[0]["agents"]["a1"]["seen_fraction"] == 3 / 7 and s[0]["agents"]["a1"]["top_cell"] == (4, 3) and s[0]["agents"]["a1"]["top_hidden_cell"] == (4, 3)
    assert s[1]["agents"]["a0"]["seen_fraction"] == 0.0 and s[1]["agents"]["a0"]["spawns"] == 0
    tr.clear()
    assert all(int(v.sum()) == 0 for v in tr.counts().values())


@pytest.mark.parametrize("shape", [(9, 7, 3, 2, 5, 3, 40, 30, 3), (6, 5, 4, 1, 7, 8, 33, 17, 2), (5, 3, 2, 2, 4, 1, 9, 9, 1)], ids=str)
def test_random_streams_equal_the_loop_and_keep_the_invariants(shape):
    T, N, A, n_cops, R, cell, W, H, G = shape
    pos, term, obs, group, quota = synthetic_stream(11, T, N, A, R, W, H, G)
    Wc, Hc = grid_shape((W, H), cell)
    for with_obs in (True, False):
        tr = _tracker(N, A, n_cops, W, H, cell, G)
        tr.set_groups(group)
        tr.set_quota(quota)
        _feed(tr, pos, term, obs if with_obs else None)
        got = tr.counts()
        _assert_equal(got, loop_reference(pos, term, obs if with_obs else None, group, quota, n_cops, cell, Wc, Hc, G), with_obs)
        c = got["counts"]
        for g in range(G):
            assert c[g, OCC].sum() + c[g, SPAWN].sum() + got["outside"][g].sum() == got["rows"][g] * A
        assert (c[:, SEEN] <= c[:, OCC]).all() and (c >= 0).all()
    # no groups, no quota: every row of every slot counts in group 0
    tr = _tracker(N, A, n_cops, W, H, cell, 1)
    _feed(tr, pos, term, obs)
    _assert_equal(tr.counts(), loop_reference(pos, term, obs, None, None, n_cops, cell, Wc, Hc, 1))
    assert tr.counts()["rows"][0] == T * N


def test_chunking_invariance():
    T, N, A, n_cops, R, cell, W, H, G = 12, 9, 3, 2, 6, 4, 50, 20, 2
    pos, term, obs, group, quota = synthetic_stream(5, T, N, A, R, W, H, G)
    trackers = [_tracker(N, A, n_cops, W, H, cell, G) for _ in range(3)]
    for tr in trackers:
        tr.set_groups(group)
        tr.set_quota(quota)
    _feed(trackers[0], pos, term, obs)
    _feed(trackers[1], pos, term, obs, one_by_one=True)
    _feed(trackers[2], pos[:5], term[:5], obs[:5])
    _feed(trackers[2], pos[5:], term[5:], obs[5:])
    for tr in trackers[1:]:
        _assert_equal(tr.counts(), trackers[0].counts())


def test_groups_by_segment_bounds_and_bad_arguments():
    tr = _tracker(8, 2, 1, 16, 16, 4, G=3)
    tr.set_groups(bounds=[0, 3, 8])
    assert tr.tensors()["group"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    tr.set_groups([2, -1, 0, 1, 2, 2, 0, -1])
    assert tr.tensors()["group"].tolist() == [2, -1, 0, 1, 2, 2, 0, -1]
    tr.set_groups()
    assert tr.tensors()["group"].tolist() == [0] * 8
    for bad in ([0] * 7, [3] + [0] * 7, [-2] + [0] * 7):
        with pytest.raises(ValueError):
            tr.set_groups(bad)
    with pytest.raises(ValueError):
        tr.set_groups(bounds=[0, 2, 4, 6, 8])               # four segments, three groups
    with pytest.raises(ValueError):
        tr.set_groups(bounds=[0, 9])
    with pytest.raises(ValueError):
        tr.update(torch.zeros(8, 3, 2, dtype=torch.float16), torch.zeros(8, dtype=torch.uint8))
    for kw in ({"cell": 0}, {"cell": 2.0}, {"G": 0}):
        with pytest.raises(ValueError):
            _tracker(4, 2, 1, 16, 16, kw.get("cell", 4), kw.get("G", 1))
    with pytest.raises(ValueError):
        _tracker(4, 17, 1, 16, 16, 4)


# ---------------------------------------------------------------------------------------------- 2. header <-> library <-> ctypes
def test_positions_header_matches_the_library_and_the_ctypes_mirror():
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.build()
    L = ln.lib()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_render.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct cat_render_positions_args \{(.*?)\} cat_render_positions_args;", code, re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in ln.PositionsArgs._fields_], names
    assert C.sizeof(ln.PositionsArgs) == 10 * 4 + 9 * 8
    assert hasattr(L, "cat_render_positions_update") and "cat_render_positions_update" in ln.MODULES["cat_render"][1]
    assert L.cat_render_abi_version() == 1
    for name, value in (("OCC", ln.POSITIONS_OCC), ("SEEN", ln.POSITIONS_SEEN), ("SPAWN", ln.POSITIONS_SPAWN), ("MAX_TICKS", ln.POSITIONS_MAX_TICKS)):
        assert re.search(r"#define CAT_POSITIONS_%s %d\b" % (name, value), code), name
    assert (OCC, SEEN, SPAWN) == (0, 1, 2)


def test_positions_update_refuses_bad_arguments_before_touching_a_device():
    """Every call below must come back with -1 and a message and never reach a HIP call (there is no device here; the fake device
    pointers are never dereferenced)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    fake = 0x1000

    def args(**kw):
        a = ln.PositionsArgs(4, 8, 3, 2, 16, 8, 5, 4, 2, 0, fake, fake, fake, fake, fake, fake, fake, fake, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejects(a, what):
        assert L.cat_render_positions_update(C.byref(a), None) == -1
        msg = L.cat_render_last_error().decode()
        assert msg.startswith("cat_render_positions_update:") and what in msg, msg

    assert L.cat_render_positions_update(None, None) == -1 and L.cat_render_last_error().decode().startswith("cat_render_positions_update:")
    for kw in ({"T": 0}, {"T": 65537}, {"N": 0}, {"A": 0}, {"A": 17}, {"n_cops": 4}, {"n_cops": -1}):
        rejects(args(**kw), "dimensions")
    rejects(args(cell=0), "cell")
    rejects(args(cell=-3), "cell")
    rejects(args(Wc=0), "grid")
    rejects(args(Hc=0), "grid")
    rejects(args(G=0), "G must be")
    for name in ("counts", "team_positions", "terminated", "outside", "rows", "done"):
        rejects(args(**{name: 0}), "NULL")
    rejects(args(team_positions=fake + 2), "aligned")
    rejects(args(R=0), "R >= 1")


# ---------------------------------------------------------------------------------------------- 3. the heatmap
def _walled_map(W=12, H=8) -> CompiledMap:
    """One axis-aligned wall, the box [8, 10] x [2, 4], as four planes."""
    planes = np.zeros((4, PLANE_STRIDE))
    for k, (nx, ny, d) in enumerate(((1, 0, 10), (-1, 0, -8), (0, 1, 4), (0, -1, -2))):
        planes[k, 0], planes[k, 1], planes[k, 4] = nx, ny, d
    return CompiledMap(name="walled", window=(float(W), float(H)), shape_bb=np.array([[8.0, 2.0, 10.0, 4.0]]), shape_first=np.zeros(1, np.int32),
                       shape_count=np.full(1, 4, np.int32), planes=planes, start_pos=np.zeros((2, 2)), region_off=np.zeros(3, np.int32),
                       regions=np.zeros((0, 4)), n_cops=1, n_thieves=1)


def test_render_heatmap_gives_the_palette_bytes_and_keeps_the_walls_grey():
    cm = _walled_map()
    plane = np.array([[0, 0], [5, 0], [10, 0]], np.int64)              # 3 cells along x, cell = 4: levels 0, 127, 255 in row 0
    img = render_heatmap(cm, plane, 4)
    assert img.shape == (12, 8, 3) and img.dtype == np.uint8
    assert (img[0:4, 0:4] == HEAT_PALETTE[0]).all() and (img[4:8, 0:4] == HEAT_PALETTE[5 * 255 // 10]).all()
    assert (HEAT_PALETTE[0] == 255).all() and 5 * 255 // 10 == 127
    grey = np.zeros((12, 8), bool)
    grey[7:12, 1:6] = True                                              # pixel centres within 1 of the box (the hull is inflated by 1)
    from as_cops_and_thieves_amd.render import render_rgb_array
    walls = (render_rgb_array(cm, np.zeros((0, 2)), 0, 0.0) == 60).all(axis=2)
    assert walls.any() and (walls <= grey).all()
    assert (img[walls] == 60).all()
    top = (~walls)[8:12, 0:4]
    assert top.any() and (img[8:12, 0:4][top] == HEAT_PALETTE[255]).all()
    assert (img[:, 4:8][~walls[:, 4:8]] == HEAT_PALETTE[0]).all()
    # vmax: given, saturating, and zero
    assert (render_heatmap(cm, plane, 4, vmax=20)[4:8, 0:4] == HEAT_PALETTE[5 * 255 // 20]).all()
    assert (render_heatmap(cm, plane, 4, vmax=2)[4:8, 0:4] == HEAT_PALETTE[255]).all()
    assert (render_heatmap(cm, plane, 4, vmax=0)[0:8, 0:4] == HEAT_PALETTE[0]).all()
    assert (render_heatmap(cm, np.zeros((3, 2), np.int64), 4)[0:8] == HEAT_PALETTE[0]).all()
    with pytest.raises(ValueError):
        render_heatmap(cm, plane[:2], 4)                                # the plane does not cover the window


def test_write_heatmaps_writes_the_pictures_and_the_counts(tmp_path):
    pos, term, obs, group, quota = _hand_built()
    tr = _tracker(4, 2, 1, 40, 30, 8, G=2)
    tr.set_groups(group)
    _feed(tr, pos, term, obs)
    cm = CompiledMap(name="empty", window=(40.0, 30.0), shape_bb=np.zeros((0, 4)), shape_first=np.zeros(0, np.int32), shape_count=np.zeros(0, np.int32),
                     planes=np.zeros((0, PLANE_STRIDE)), start_pos=np.zeros((2, 2)), region_off=np.zeros(3, np.int32), regions=np.zeros((0, 4)),
                     n_cops=1, n_thieves=1)
    c = write_heatmaps(tmp_path / "hm", tr, cm, group_names=["first", None])
    files = sorted(p.relative_to(tmp_path / "hm").as_posix() for p in (tmp_path / "hm").rglob("*") if p.is_file())
    assert files == sorted([f"first/a{i}_{p}.png" for i in range(2) for p in ("occ", "seen", "hidden", "spawn")] + ["positions.npz"])
    z = np.load(tmp_path / "hm" / "positions.npz")
    assert np.array_equal(z["counts"], c["counts"]) and np.array_equal(z["rows"], c["rows"]) and int(z["cell"]) == 8
    assert z["agents"].tolist() == ["a0", "a1"] and z["groups"].tolist() == ["first", ""]
    assert (tmp_path / "hm" / "first" / "a0_occ.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


# ---------------------------------------------------------------------------------------------- 4. the env hook
class PositionedOracleVecEnv(OracleVecEnv):
    """The CPU stand-in env with what ``VecCopsEnv(track_positions=CELL)`` adds: after every step ``VecCopsEnv._track`` itself is run
    on the oracle's buffers (which, after the stand-in's auto-reset, hold what the device buffers hold)."""

    def __init__(self, cmap, num_envs, cell, **kw):
        super().__init__(cmap, num_envs, **kw)
        self._tracker, self._exposure = None, True
        self._positions = PositionTracker(num_envs, self.possible_agents, cmap.n_cops, (int(cmap.window[0]), int(cmap.window[1])), cell)
        self.recorded = []

    def step(self, actions):
        from as_cops_and_thieves_amd.environments import VecCopsEnv
        res = super().step(actions)
        o = self.sim.out
        out = {"team_positions": torch.from_numpy(o["team_positions"].view(np.float16).copy()), "obs_type": torch.from_numpy(o["obs_type"].copy()),
               "terminated": res[2][self.possible_agents[0]].to(torch.uint8)}
        self.recorded.append(out)
        VecCopsEnv._track(self, out)
        return res


def test_a_tracked_env_counts_what_the_cpu_tracker_counts_on_the_recorded_rows():
    cmap = load_preset("squarinth").compile()
    N, cell = 6, 16
    env = PositionedOracleVecEnv(cmap, N, cell, num_rays=16, max_step_count=7, seed=3)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        env.step(torch.from_numpy(rng.integers(0, 4, size=(N, len(env.possible_agents))).astype(np.int32)))
    rows = {k: torch.stack([r[k] for r in env.recorded]) for k in env.recorded[0]}
    twin = PositionTracker(N, env.possible_agents, cmap.n_cops, (int(cmap.window[0]), int(cmap.window[1])), cell)
    twin.update(rows["team_positions"], rows["terminated"], rows["obs_type"])
    got = env._positions.counts()
    _assert_equal(got, twin.counts())
    _assert_equal(got, loop_reference(rows["team_positions"].numpy(), rows["terminated"].numpy(), rows["obs_type"].numpy(), None, None, cmap.n_cops,
                                      cell, twin.Wc, twin.Hc, 1))
    assert got["rows"][0] == 20 * N and got["counts"][0, SPAWN].sum() >= 2 * N * len(env.possible_agents) and got["outside"].sum() == 0


def test_track_positions_needs_auto_reset_and_a_cell_size():
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    with pytest.raises(ValueError, match="auto_reset"):
        VecCopsEnv(load_preset("squarinth"), 8, auto_reset=False, track_positions=8)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="track_positions"):
            VecCopsEnv(load_preset("squarinth"), 8, track_positions=bad)
