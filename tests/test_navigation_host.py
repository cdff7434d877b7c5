"""Navigation without a GPU: the NumPy tables of ``navigation`` (free / snap / hops) against values written out by hand, the torch tick
``navigate_step`` walking on a grid with no physics and on explicit rows, the bundled maps, the C ABI of ``cat_render_nav_build`` /
``cat_render_nav_step`` with their argument checks (which come before any device call), and ``NavigatorActor`` on the oracle-backed
stand-in env."""
import ctypes as C
import json
import re
from collections import deque
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd import navigation as nv
from as_cops_and_thieves_amd.maps import MAPS_DIR, PLANE_STRIDE, CompiledMap, _planes_for_hull, convex_hull, load_preset
from tests.fake_env import OracleVecEnv
from tests.navigation_cases import (GOAL_00, MASK_7X5, OPEN_13X9, SPARSE_6X6, centre, explicit_rows, index, mask_of)

ROOT = Path(__file__).resolve().parents[1]
NONE = nv.NONE


# ---------------------------------------------------------------------------------------------- 1. free and snap by hand
def _rectangle_map(x0=95.0, y0=87.0, w=100.0, h=60.0, W=320.0, H=240.0) -> CompiledMap:
    """One rectangle hull [x0, x0 + w] x [y0, y0 + h] in a W x H window."""
    hull = convex_hull([(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)])
    planes = _planes_for_hull(hull)
    assert planes.shape == (4, PLANE_STRIDE)
    return CompiledMap(name="rect", window=(W, H), shape_bb=np.array([[x0 - 1, y0 - 1, x0 + w + 1, y0 + h + 1]]), shape_first=np.zeros(1, np.int32),
                       shape_count=np.full(1, 4, np.int32), planes=planes, start_pos=np.zeros((2, 2)), region_off=np.zeros(3, np.int32),
                       regions=np.zeros((0, 4)), n_cops=1, n_thieves=1)


def test_free_and_snap_around_a_rectangle_at_cell_16():
    """Rectangle [95, 195] x [87, 147], clearance 6, cell 16: centres at 8 + 16 i.  Blocked: x centres 104 .. 200 (ix 6 .. 12; 200 is 5 off
    the right edge), y centres 88 .. 152 (iy 5 .. 9; 152 is 5 above the top edge) -- but not (12, 9): its centre (200, 152) is sqrt(50) > 6
    from the corner (195, 147).  A square inflation would block it; the Euclidean rule does not."""
    free, Wc, Hc = nv.free_cells(_rectangle_map(), 16, 6.0)
    assert (Wc, Hc) == (20, 15) and free.dtype == np.uint8 and free.shape == (300,)
    want = np.ones((20, 15), np.uint8)
    want[6:13, 5:10] = 0
    want[12, 9] = 1
    assert np.array_equal(free.reshape(20, 15), want)
    snap = nv.snap_cells(free, Wc, Hc)
    assert snap.dtype == np.uint16 and np.array_equal(snap[free != 0], np.arange(300)[free != 0])
    k = lambda ix, iy: ix * 15 + iy
    assert snap[k(6, 5)] == k(5, 5)                    # the block's corner: distance 1 to (5, 5) and (6, 4), the lower index wins
    assert snap[k(7, 5)] == k(7, 4)                    # (6, 5) is blocked, (7, 4) is the next offset in the order
    assert snap[k(11, 8)] == k(12, 9)                  # only the free corner cell is within reach at distance sqrt(2)
    assert snap[k(8, 6)] == k(8, 4)                    # two rings away: (6, 6) is blocked, (8, 4) is free
    assert snap[k(12, 7)] == k(13, 7) and snap[k(9, 9)] == k(9, 10)
    for ix, iy in ((8, 7), (9, 7)):                    # more than two rings from any free cell
        assert snap[k(ix, iy)] == NONE
    assert snap[k(10, 7)] == k(12, 9) and int((snap == NONE).sum()) == 2      # (10, 7) just reaches the free corner cell
    # the window rule: with clearance 9 the outermost ring of cells (centres 8 from the border) goes too
    ring, _, _ = nv.free_cells(_rectangle_map(), 16, 9.0)
    ring = ring.reshape(20, 15)
    assert not ring[0].any() and not ring[-1].any() and not ring[:, 0].any() and not ring[:, -1].any() and ring[1, 1] and ring[18, 13]


def test_free_and_snap_around_a_rectangle_at_cell_20():
    """Cell 20: centres at 10 + 20 i.  Blocked: x centres 90 .. 190 (ix 4 .. 9; 90 is 5 left of the edge), y centres 90 .. 150 (iy 4 .. 7;
    150 is 3 above the top); the corner cell (4, 7) at (90, 150) is sqrt(34) < 6 from (95, 147): blocked too."""
    free, Wc, Hc = nv.free_cells(_rectangle_map(), 20, 6.0)
    assert (Wc, Hc) == (16, 12)
    want = np.ones((16, 12), np.uint8)
    want[4:10, 4:8] = 0
    assert np.array_equal(free.reshape(16, 12), want)
    snap = nv.snap_cells(free, Wc, Hc)
    k = lambda ix, iy: ix * 12 + iy
    assert snap[k(4, 4)] == k(3, 4) and snap[k(6, 5)] == k(6, 3) and snap[k(6, 6)] == k(6, 8) and int((snap == NONE).sum()) == 0
    with pytest.raises(ValueError):
        nv.free_cells(_rectangle_map(W=1300.0, H=1300.0), 16, 6.0)       # 82 x 82 cells
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError):
            nv.grid_shape((320, 240), bad)


# ---------------------------------------------------------------------------------------------- 2. the hop table
def _bfs_table(free, Wc, Hc):
    """A plain queue per goal: an independent statement of the table."""
    Cn = Wc * Hc
    out = np.full((Cn, Cn), NONE, np.uint16)
    for g in range(Cn):
        if not free[g]:
            continue
        seen, q = {g: 0}, deque([g])
        while q:
            k = q.popleft()
            ix, iy = divmod(k, Hc)
            for jx, jy in ((ix - 1, iy), (ix + 1, iy), (ix, iy - 1), (ix, iy + 1)):
                j = jx * Hc + jy
                if 0 <= jx < Wc and 0 <= jy < Hc and free[j] and j not in seen:
                    seen[j] = seen[k] + 1
                    q.append(j)
        for k, v in seen.items():
            out[g, k] = v
    return out


def test_hops_reference_on_the_7x5_mask():
    free, Wc, Hc = MASK_7X5
    hops = nv.hops_reference(free, Wc, Hc)
    assert hops.dtype == np.uint16 and hops.shape == (35, 35)
    assert np.array_equal(hops[index(0, 0, Hc)], GOAL_00)                      # the row written out by hand
    pocket = np.full(35, NONE, np.uint16)
    pocket[index(6, 1, Hc)], pocket[index(6, 2, Hc)] = 0, 1
    assert np.array_equal(hops[index(6, 1, Hc)], pocket)                       # the enclosed pocket sees itself only
    assert (hops[index(3, 0, Hc)] == NONE).all() and (hops[:, index(3, 0, Hc)] == NONE).all()     # a blocked goal, a blocked cell
    assert np.array_equal(hops, hops.T)
    assert np.array_equal(hops, _bfs_table(free, Wc, Hc))
    assert np.array_equal(nv.hops_reference(free, Wc, Hc, goals=[34, 0, 7]), hops[[34, 0, 7]])
    assert nv.component_sizes(free, Wc, Hc) == [20, 2]


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (13, 9), (11, 6)], ids=str)
def test_hops_reference_equals_a_queue_per_goal(shape):
    Wc, Hc = shape
    free = (np.random.default_rng(Wc * 100 + Hc).random(Wc * Hc) > (0.3 if shape == (11, 6) else 0.0)).astype(np.uint8)
    hops = nv.hops_reference(free, Wc, Hc)
    assert np.array_equal(hops, _bfs_table(free, Wc, Hc)) and np.array_equal(hops, hops.T)


# ---------------------------------------------------------------------------------------------- 3. the tick
def _walk_field(n):
    return nv.NavField(16, [MASK_7X5], np.zeros(n, np.int32))


ACTION_STEP = ((-1, 0), (0, 1), (1, 0), (0, -1))       # 0 = -x, 1 = +y, 2 = +x, 3 = -y


def _pairs():
    free, Wc, Hc = MASK_7X5
    hops = nv.hops_reference(free, Wc, Hc).astype(np.int64)
    a, b = np.nonzero((hops != NONE) & (hops > 0))
    return hops, a, b, Hc


def _positions(cells, Hc):
    """f16 [n, 2]: the centres of the cells, at cell 16."""
    return torch.tensor([centre(k // Hc, k % Hc) for k in cells], dtype=torch.float16)


def test_pursue_walks_every_shortest_path_on_the_grid():
    """From every free cell towards every reachable goal: each action leads to a neighbour exactly one hop nearer, and the walk arrives in
    hops steps.  The walker is moved from cell centre to cell centre: no physics."""
    hops, goal, start, Hc = _pairs()
    n = len(start)
    assert n == 20 * 19 + 2
    field = _walk_field(n)
    cur = start.copy()
    u = torch.full((1, n), 0.5)
    for step in range(int(hops[goal, start].max())):
        tp = torch.stack([_positions(cur, Hc), _positions(goal, Hc)], dim=1)
        act, nav = nv.navigate_step(tp, u, field, [0], [nv.PURSUE], [0b10])
        act, nav = act[0].numpy(), nav[0].numpy()
        there = cur == goal
        assert np.array_equal(nav, hops[goal, cur])
        nxt = np.array([k if t else (k // Hc + ACTION_STEP[a][0]) * Hc + k % Hc + ACTION_STEP[a][1] for k, a, t in zip(cur, act, there)])
        assert (hops[goal, nxt][~there] == hops[goal, cur][~there] - 1).all(), step
        assert (there == (hops[goal, start] <= step)).all()                  # arrival after exactly hops steps, not before
        cur = np.where(there, cur, nxt)
    assert (cur == goal).all()


def test_flee_never_picks_a_neighbour_with_a_smaller_minimum():
    hops, cop, thief, Hc = _pairs()
    free, Wc, _ = MASK_7X5
    n = len(thief)
    tp = torch.stack([_positions(cop, Hc), _positions(thief, Hc)], dim=1)
    act, nav = nv.navigate_step(tp, torch.full((1, n), 0.5), _walk_field(n), [1], [nv.FLEE], [0b01])
    assert np.array_equal(nav[0].numpy(), hops[cop, thief])
    for c, t, a in zip(cop, thief, act[0].tolist()):
        ix, iy = divmod(t, Hc)
        usable = {i: (ix + dx) * Hc + iy + dy for i, (dx, dy) in enumerate(ACTION_STEP)
                  if 0 <= ix + dx < Wc and 0 <= iy + dy < Hc and free[(ix + dx) * Hc + iy + dy]}
        assert a in usable and hops[c, usable[a]] == max(hops[c, k] for k in usable.values())
        assert a == min(i for i, k in usable.items() if hops[c, k] == hops[c, usable[a]])     # one opponent: equal sums, the lowest action


def test_explicit_rows_tie_breaks_fallback_and_the_same_cell():
    """``tests/navigation_cases.explicit_rows``: every row carries its answer, derived by hand from the rule's text."""
    rows = explicit_rows()
    tp = torch.tensor([r["pos"] for r in rows], dtype=torch.float16)
    u = torch.tensor([[r["u"] for r in rows]] * 2, dtype=torch.float32)
    field = nv.NavField(16, [MASK_7X5, OPEN_13X9, SPARSE_6X6], [r["map"] for r in rows])
    script = torch.tensor([[nv.PURSUE if r["pursue"] is not None else -1 for r in rows], [nv.FLEE if r["flee"] is not None else -1 for r in rows]])
    act, nav = nv.navigate_step(tp, u, field, [0, 2], script, [0b100, 0b011])
    for i, r in enumerate(rows):
        for g, key in enumerate(("pursue", "flee")):
            want = (-1, -1) if r[key] is None else r[key]
            assert (int(act[g, i]), int(nav[g, i])) == want, (r["name"], key, int(act[g, i]), int(nav[g, i]))
    assert act.dtype == torch.int32 and nav.dtype == torch.int32
    names = {r["name"] for r in rows}
    assert {"nan", "negative", "pocket", "same cell x", "same cell y", "tie pref x", "tie pref y", "pref outside", "snapped", "no snap",
            "flee lowest", "flee sum"} <= names


# ---------------------------------------------------------------------------------------------- 4. the bundled maps
def _segment_distance(points, a, b):
    """Distance of points [P, 2] to the segment a -> b, by the closest-point form (not the projection-residual form of the module)."""
    e = b - a
    t = np.clip(((points - a) @ e) / (e @ e), 0.0, 1.0)
    closest = a + t[:, None] * e
    return np.hypot(points[:, 0] - closest[:, 0], points[:, 1] - closest[:, 1])


@pytest.mark.parametrize("name", sorted(json.loads((MAPS_DIR / "presets.json").read_text())))
def test_bundled_maps_fit_the_grid_and_free_cells_clear_the_walls(name):
    cm = load_preset(name).compile()
    free, Wc, Hc = nv.free_cells(cm, 16, 6.0)
    assert Wc * Hc <= nv.MAX_CELLS
    k = np.nonzero(free)[0]
    pts = np.stack([(k // Hc + 0.5) * 16, (k % Hc + 0.5) * 16], axis=1)
    nearest = np.full(len(k), np.inf)
    for first, count in zip(cm.shape_first, cm.shape_count):
        v = cm.planes[first:first + count, 2:4]
        for i in range(count):
            nearest = np.minimum(nearest, _segment_distance(pts, v[i - 1], v[i]))
    assert len(k) > 0 and nearest.min() > 6.0, (name, nearest.min())
    print(f"{name}: {Wc} x {Hc} = {Wc * Hc} cells, {len(k)} free, components {nv.component_sizes(free, Wc, Hc)[:10]}, "
          f"cells without a snap {int((nv.snap_cells(free, Wc, Hc) == NONE).sum())}, nearest wall {nearest.min():.3f}")


# ---------------------------------------------------------------------------------------------- 5. header <-> library <-> ctypes
def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_render.h").read_text(), flags=re.S)


def _fields(code, struct_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), code, re.S).group(1)
    body = re.sub(r"\[[^\]]*\]", "", body)
    return [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]


def test_nav_header_matches_the_library_and_the_ctypes_mirrors():
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.build()
    L = ln.lib()
    code = _header()
    assert _fields(code, "cat_render_nav_build_args") == [f[0] for f in ln.NavBuildArgs._fields_]
    assert _fields(code, "cat_render_nav_step_args") == [f[0] for f in ln.NavStepArgs._fields_]
    assert C.sizeof(ln.NavBuildArgs) == 2 * 4 + 4 * 8
    assert C.sizeof(ln.NavStepArgs) == (6 + 8 + 8 + 33 + 1 + 8 * 32) * 4 + 9 * 8
    for sym in ("cat_render_nav_build", "cat_render_nav_step"):
        assert hasattr(L, sym) and sym in ln.MODULES["cat_render"][1] and re.search(r"\bint %s\(" % sym, code)
    assert list(ln.MODULES["cat_render"][1])[:3] == ["cat_render_frames", "cat_render_positions_update", "cat_render_positions_ends_update"]
    assert L.cat_render_abi_version() == 1 and ln.MODULES["cat_render"][0] == 1 and "#define CAT_RENDER_ABI_VERSION 1" in code
    for name, value in (("MAX_CELLS", ln.NAV_MAX_CELLS), ("MAX_MAPS", ln.NAV_MAX_MAPS), ("MAX_NAVIGATORS", ln.NAV_MAX_NAVIGATORS),
                        ("MAX_SEGMENTS", ln.NAV_MAX_SEGMENTS), ("PURSUE", ln.NAV_PURSUE), ("FLEE", ln.NAV_FLEE)):
        assert re.search(r"#define CAT_NAV_%s %d\b" % (name, value), code), name
    assert "#define CAT_NAV_NONE 0xFFFF" in code and ln.NAV_NONE == nv.NONE == 0xFFFF
    assert (nv.MAX_CELLS, nv.MAX_MAPS, nv.PURSUE, nv.FLEE) == (ln.NAV_MAX_CELLS, ln.NAV_MAX_MAPS, ln.NAV_PURSUE, ln.NAV_FLEE)
    assert ln.PKG / "csrc" / "cat_render_nav.h" in ln.INTERNAL_HEADERS and len(ln.SOURCES) == 8


def _rejected(L, entry, a, what, seen):
    assert getattr(L, entry)(None if a is None else C.byref(a), None) == -1
    msg = L.cat_render_last_error().decode()
    assert msg.startswith(entry + ":") and what in msg, msg
    seen.add(msg)


def test_nav_build_refuses_bad_arguments_before_touching_a_device():
    """Every call must come back with -1 and a message of its own and never reach a HIP call (there is no device here; the fake device
    pointers are never dereferenced)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    fake = 0x1000
    grid = np.array([[7, 5, 0, 0], [13, 9, 35, 1225]], np.int32)

    def args(g=grid, **kw):
        a = ln.NavBuildArgs(len(g), 0, g.ctypes.data, fake, fake, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    seen = set()
    _rejected(L, "cat_render_nav_build", None, "NULL arguments", seen)
    for n in (0, -1, 17):
        _rejected(L, "cat_render_nav_build", args(n_maps=n), "n_maps", seen)
    for name in ("grid_host", "grid"):
        _rejected(L, "cat_render_nav_build", args(**{name: 0}), "grid table", seen)
    for name in ("free", "hops"):
        _rejected(L, "cat_render_nav_build", args(**{name: 0}), "buffer is NULL", seen)
    _rejected(L, "cat_render_nav_build", args(hops=fake + 1), "aligned", seen)
    _rejected(L, "cat_render_nav_build", args(np.array([[0, 5, 0, 0]], np.int32)), "Wc >= 1", seen)
    _rejected(L, "cat_render_nav_build", args(np.array([[65, 64, 0, 0]], np.int32)), "4096", seen)
    _rejected(L, "cat_render_nav_build", args(np.array([[7, 5, 0, 0], [13, 9, 36, 1225]], np.int32)), "offsets", seen)
    _rejected(L, "cat_render_nav_build", args(np.array([[7, 5, 0, 0], [13, 9, 35, 1224]], np.int32)), "offsets", seen)
    assert len(seen) == 8


def test_nav_step_refuses_bad_arguments_before_touching_a_device():
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    fake = 0x1000
    table = ln.nav_table(70, 2, [0, 30, 70], [[0, -1], [1, 1]])

    def args(**kw):
        a = ln.NavStepArgs(70, 3, 2, 2, 1, 16, (C.c_int32 * 8)(0, 2), (C.c_uint32 * 8)(0b100, 0b011), table.seg_start, 0, table.seg_script,
                           fake, fake, fake, fake, fake, fake, fake, fake, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    seen = set()
    rej = lambda a, what: _rejected(L, "cat_render_nav_step", a, what, seen)
    rej(None, "NULL arguments")
    for kw in ({"N": 0}, {"A": 0}, {"A": 17}):
        rej(args(**kw), "dimensions")
    for g in (0, 9):
        rej(args(G=g), "G must")
    for s in (0, 33):
        rej(args(S=s), "S must")
    for n in (0, 17):
        rej(args(n_maps=n), "n_maps")
    rej(args(cell=0), "cell")
    rej(args(agent=(C.c_int32 * 8)(0, 3)), "agent index")
    rej(args(agent=(C.c_int32 * 8)(-1, 2)), "agent index")
    rej(args(opp_mask=(C.c_uint32 * 8)(0b1100, 0b011)), "opp_mask")          # agent 3 of 3
    rej(args(opp_mask=(C.c_uint32 * 8)(0b101, 0b011)), "opp_mask")           # the navigator itself
    rej(args(seg_start=(C.c_int32 * 33)(1, 30, 70)), "begin at 0")
    rej(args(seg_start=(C.c_int32 * 33)(0, 30, 69)), "end at N")
    rej(args(seg_start=(C.c_int32 * 33)(0, 70, 70)), "strictly increasing")
    bad = ln.nav_table(70, 2, [0, 30, 70], [[0, -1], [1, 1]])
    bad.seg_script[1][1] = 2
    rej(args(seg_script=bad.seg_script), "script outside")
    for name in ("grid", "free", "snap", "hops"):
        rej(args(**{name: 0}), "table of the field")
    for name in ("team_positions", "uniform", "actions"):
        rej(args(**{name: 0}), "buffer is NULL")
    rej(args(team_positions=fake + 2), "aligned")
    assert len(seen) == 15
    with pytest.raises(ValueError):
        ln.nav_table(70, 2, [0, 30, 70], [[0, 2], [1, 1]])
    with pytest.raises(ValueError):
        ln.nav_table(70, 2, [0, 30, 69], [[0, 0], [1, 1]])


# ---------------------------------------------------------------------------------------------- 6. the actor
class PositionedEnv(OracleVecEnv):
    """The CPU stand-in env (``tests/fake_env.py`` offers team_positions per team through ``state()`` only) with what a ``NavigatorActor``
    reads of a ``VecCopsEnv``: the compiled maps, the config, ``slot_map_ids`` and ``raw_outputs()["team_positions"]`` f16 [N, A, 2]."""

    def __init__(self, cmap, num_envs, **kw):
        super().__init__(cmap, num_envs, **kw)
        self._compiled, self._cfg = [cmap], self.cfg
        self.slot_map_ids = np.zeros(num_envs, np.int32)

    def raw_outputs(self):
        return {"team_positions": torch.from_numpy(self.sim.out["team_positions"].view(np.float16).copy())}


@pytest.fixture(scope="module")
def env_and_field():
    env = PositionedEnv(load_preset("squarinth").compile(), 6, num_rays=16, max_step_count=30, seed=3)
    env.reset()
    return env, nv.NavField.from_env(env, cell=32)     # 40 x 25 cells: a quick table on the CPU


def test_navigator_actor_refuses_what_does_not_fit(env_and_field):
    from as_cops_and_thieves_amd.selfplay.navigators import NAVIGATORS, NavigatorActor, navigator_code
    env, field = env_and_field
    assert NAVIGATORS == {"pursue": 0, "flee": 1} and navigator_code(None) == -1 and navigator_code("flee", "thief_0") == 1
    assert env.possible_agents == ["cop_0", "cop_1", "thief_0"]
    for bad in ({"cop_0": "flee"}, {"thief_0": "pursue"}, {"cop_0": "chase"}, {"cop_0": 0}, {"robber_0": "pursue"}, {}):
        with pytest.raises(ValueError):
            NavigatorActor(env, bad, field=field)
    with pytest.raises(ValueError):
        NavigatorActor(env, {"cop_0": "pursue"}, agents=["thief_0"], field=field)
    with pytest.raises(ValueError):
        NavigatorActor(env, {"cop_0": "pursue"}, field=nv.NavField(32, [MASK_7X5], np.zeros(5, np.int32)))      # a field of another batch
    actor = NavigatorActor(env, {"cop_0": "pursue"}, agents=["cop_0", "thief_0"], field=field)
    table = actor.table
    for bad in ([], [(0, 4, {"cop_0": "pursue", "thief_0": "flee"})], [(0, 3, {"cop_0": None, "thief_0": "flee"}), (4, 6, {"cop_0": None, "thief_0": None})],
                [(1, 6, {"cop_0": "pursue", "thief_0": "flee"})], [(0, 6, {"cop_0": "pursue"})], [(0, 6, {"cop_0": "flee", "thief_0": "flee"})]):
        with pytest.raises(ValueError):
            actor.set_segments(bad)
    assert actor.table is table                        # a refused table leaves the current one
    actor.set_segments([(0, 2, {"cop_0": "pursue", "thief_0": None}), (2, 6, {"cop_0": None, "thief_0": "flee"})])
    assert actor.table is not table and actor.segments == [(0, 2), (2, 6)]


def test_navigator_actor_writes_its_own_columns_only(env_and_field):
    from as_cops_and_thieves_amd.selfplay.navigators import NavigatorActor
    env, field = env_and_field
    actor = NavigatorActor(env, agents=["cop_0", "thief_0"], field=field)
    assert not actor.fused and actor.agents == ["cop_0", "thief_0"] and actor.indices == [0, 2] and actor.opponent_masks == [0b100, 0b011]
    assert actor.N == 6 and actor.env_agents == env.possible_agents and actor.get_state().numel() == 0
    actor.set_segments([(0, 2, {"cop_0": "pursue", "thief_0": None}), (2, 6, {"cop_0": None, "thief_0": "flee"})])
    actor.reset(); actor.set_state(actor.get_state())
    torch.manual_seed(3)
    for tick in range(8):
        u = torch.rand(2, 6)
        actions = torch.full((6, 3), 9, dtype=torch.int32)
        assert actor.act(env, uniform=u, actions=actions) is actions
        script = torch.tensor([[0, 0, -1, -1, -1, -1], [-1, -1, 1, 1, 1, 1]])
        want, hops = nv.navigate_step(env.raw_outputs()["team_positions"], u, field, [0, 2], script, [0b100, 0b011])
        assert bool((actions[:, 1] == 9).all()) and bool((actions[2:, 0] == 9).all()) and bool((actions[:2, 2] == 9).all())
        assert torch.equal(actions[:2, 0], want[0, :2]) and torch.equal(actions[2:, 2], want[1, 2:]) and torch.equal(actor.nav_hops, hops)
        assert bool(((actions[:2, 0] >= 0) & (actions[:2, 0] <= 3)).all()) and bool((hops[0, :2] > 0).all())     # squarinth's spawns are connected
        actions[:, 1] = 0
        actions[2:, 0] = 1
        actions[:2, 2] = 2
        env.step(actions)
    with pytest.raises(ValueError):
        actor.act(env, actions=torch.zeros(6, 3, dtype=torch.int64))
