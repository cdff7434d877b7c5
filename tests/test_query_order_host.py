"""Tree order (``bbtree_gate = 2``, ``query_order="chipmunk"``) on the host, without a GPU: the static tree the library builds for a
map (``cat_bbtree_host``) against an independent restatement of Chipmunk's insert rule, the candidate tables of tree order
(rules 1 and 2 only) against the oracle's single-wall queries, and the option checks of the Python envs."""
import ctypes as C
import json

import numpy as np
import pytest

from as_cops_and_thieves_amd import _native as nat
from as_cops_and_thieves_amd import tables
from as_cops_and_thieves_amd.config import C_FIELDS_F64, C_FIELDS_I32, SimConfig
from as_cops_and_thieves_amd.maps import Map, load_preset

PRESETS = ("squarinth", "lbirinth", "grandbyrinth", "labyrinth", "agh-map")


def _lib():
    nat.build()
    return nat.lib()


def _random_map(tmp_path, seed, n_walls):
    """Random convex polygons and rectangles, some overlapping, some sharing coordinates (equal insertion costs)."""
    rng = np.random.default_rng(seed)
    blocks = []
    for q in range(n_walls):
        x, y = (float(v) for v in rng.integers(20, 1200, 2))
        if q % 3 == 0:
            blocks.append({"type": "rect", "x": x, "y": y, "w": float(rng.integers(2, 90)), "h": float(rng.integers(2, 90))})
        else:
            ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 9))))
            rad = rng.uniform(5, 60)
            blocks.append({"type": "poly", "vs": [{"x": x + rad * np.cos(a), "y": y + rad * np.sin(a)} for a in ang]})
    agents = [{"type": "cop", "x": 5, "y": 5}, {"type": "cop", "x": 10, "y": 5}, {"type": "thief", "x": 5, "y": 10}]
    f = tmp_path / f"random{seed}.json"
    f.write_text(json.dumps({"window": {"w_px": 1280, "h_px": 1280}, "canvas": {"w": 1280, "h": 1280},
                             "objects": {"blocks": blocks}, "agents": agents}))
    return Map(f).compile()


def _exported_tree(cmap):
    L = _lib()
    blob = cmap.to_blob()
    n = 2 * cmap.n_shapes - 1
    bb = np.zeros((n, 4), np.float64)
    link = np.zeros((n, 4), np.int32)
    root, depth = C.c_int(), C.c_int()
    got = L.cat_bbtree_host(blob, len(blob), bb.ctypes.data, link.ctypes.data, n, C.byref(root), C.byref(depth))
    assert got == n
    return bb, link, root.value, depth.value


def _restated_tree(shape_bb):
    """cpBBTreeInsert, one wall after the other in index order, written from Chipmunk's description (recursive, as SubtreeInsert)."""
    S = len(shape_bb)
    bb = [tuple(float(v) for v in shape_bb[s]) for s in range(S)]
    a, b, wall = [-1] * S, [-1] * S, list(range(S))
    lo = lambda x, y: x if x < y else y
    hi = lambda x, y: x if x > y else y
    merge = lambda x, y: (lo(x[0], y[0]), lo(x[1], y[1]), hi(x[2], y[2]), hi(x[3], y[3]))
    area = lambda x: (x[2] - x[0]) * (x[3] - x[1])
    merged_area = lambda x, y: (hi(x[2], y[2]) - lo(x[0], y[0])) * (hi(x[3], y[3]) - lo(x[1], y[1]))
    proximity = lambda x, y: abs(x[0] + x[2] - y[0] - y[2]) + abs(x[1] + x[3] - y[1] - y[3])

    def insert(sub, leaf):
        if sub < 0:
            return leaf
        if wall[sub] >= 0:
            bb.append(merge(bb[leaf], bb[sub])); a.append(leaf); b.append(sub); wall.append(-1)
            return len(bb) - 1
        ca, cb = a[sub], b[sub]
        cost_a = area(bb[cb]) + merged_area(bb[ca], bb[leaf])
        cost_b = area(bb[ca]) + merged_area(bb[cb], bb[leaf])
        if cost_a == cost_b:
            cost_a, cost_b = proximity(bb[ca], bb[leaf]), proximity(bb[cb], bb[leaf])
        if cost_b < cost_a:
            b[sub] = insert(cb, leaf)
        else:
            a[sub] = insert(ca, leaf)
        bb[sub] = merge(bb[sub], bb[leaf])
        return sub

    root = -1
    for s in range(S):
        root = insert(root, s)
    return np.array(bb, np.float64), np.array(a), np.array(b), np.array(wall), root


def _check_tree(cmap):
    bb, link, root, depth = _exported_tree(cmap)
    S = cmap.n_shapes
    rbb, ra, rb, rwall, rroot = _restated_tree(cmap.shape_bb)
    assert root == rroot
    assert bb.tobytes() == rbb.tobytes(), "node bbs bit for bit"
    assert link[:, 0].tolist() == ra.tolist() and link[:, 1].tolist() == rb.tolist() and link[:, 3].tolist() == rwall.tolist()
    # invariants: 2S - 1 nodes, S leaves (wall s at node s), every inner bb the exact merge of its children, parents, depth
    assert len(bb) == 2 * S - 1 and (link[:S, 3] == np.arange(S)).all() and (link[S:, 3] == -1).all()
    for n in range(S, 2 * S - 1):
        ca, cb = link[n, 0], link[n, 1]
        assert link[ca, 2] == n and link[cb, 2] == n
        want = np.array([min(bb[ca, 0], bb[cb, 0]), min(bb[ca, 1], bb[cb, 1]), max(bb[ca, 2], bb[cb, 2]), max(bb[ca, 3], bb[cb, 3])])
        assert bb[n].tobytes() == want.tobytes()
    assert link[root, 2] == -1
    deepest = 0
    for s in range(S):
        d, x = 0, s
        while link[x, 2] >= 0:
            x, d = link[x, 2], d + 1
        deepest = max(deepest, d)
    assert depth == deepest
    return depth


def test_static_tree_of_the_presets_is_chipmunks_insert_order():
    depths = {name: _check_tree(load_preset(name).compile()) for name in PRESETS}
    assert depths["labyrinth"] == 7 and depths["agh-map"] == 11
    assert all(3 <= d <= 11 for d in depths.values()), depths


@pytest.mark.parametrize("seed,n_walls", [(1, 1), (2, 2), (3, 17), (4, 64), (5, 200)])
def test_static_tree_of_random_maps(tmp_path, seed, n_walls):
    _check_tree(_random_map(tmp_path, seed, n_walls))


def test_static_tree_of_walls_with_equal_costs(tmp_path):
    """A row of identical squares: insertion costs tie and the proximity rule decides."""
    blocks = [{"type": "rect", "x": 40.0 * q, "y": 300, "w": 20, "h": 20} for q in range(12)]
    blocks += [{"type": "rect", "x": 500, "y": 40.0 * q, "w": 20, "h": 20} for q in range(6)]
    agents = [{"type": "cop", "x": 5, "y": 5}, {"type": "cop", "x": 10, "y": 5}, {"type": "thief", "x": 5, "y": 10}]
    f = tmp_path / "row.json"
    f.write_text(json.dumps({"window": {"w_px": 1280, "h_px": 800}, "canvas": {"w": 1280, "h": 800},
                             "objects": {"blocks": blocks}, "agents": agents}))
    _check_tree(Map(f).compile())


def _grid(cmap, cfg):
    L = _lib()
    c = nat.CatConfig()
    for n in C_FIELDS_I32 + C_FIELDS_F64:
        setattr(c, n, getattr(cfg, n))
    dx, dy = tables.ray_table(cfg.sensor)
    lut = np.zeros(32768, np.float32)
    t = nat.CatTables(dx.ctypes.data, dy.ctypes.data, lut.ctypes.data, lut.ctypes.data)
    blob = cmap.to_blob()
    h = C.c_void_p()
    assert L.cat_grid_build_host(C.byref(c), C.byref(t), blob, len(blob), 8.0, C.byref(h)) == 0
    return L, h, dx, dy


def _tbb(bb, ax, ay, bx, by):
    """[CP cpBBSegmentQuery] per wall: the thin segment's entry time into each bb (inf: missed)."""
    dx, dy = bx - ax, by - ay
    tmin = np.full(len(bb), -np.inf); tmax = np.full(len(bb), np.inf)
    ok = np.ones(len(bb), bool)
    for d, o, l, h in ((dx, ax, bb[:, 0], bb[:, 2]), (dy, ay, bb[:, 1], bb[:, 3])):
        if d == 0.0:
            ok &= ~((o < l) | (h < o))
        else:
            t1, t2 = (l - o) * (1.0 / d), (h - o) * (1.0 / d)
            tmin = np.maximum(tmin, np.minimum(t1, t2)); tmax = np.minimum(tmax, np.maximum(t1, t2))
    hit = ok & (tmin <= tmax) & (0.0 <= tmax) & (tmin <= 1.0)
    return np.where(hit, np.maximum(tmin, 0.0), np.inf)


def _check_tables(cmap, n_origins, rays=64, seed=0):
    """Every wall whose single-wall query (the oracle, this wall alone) hits -- entered by the thin segment and hit, or, for a map of one
    wall, hit at all (its root is a leaf, visited ungated) -- is on the row of the tree-order tables."""
    from oracle.cat_oracle import OracleSim
    S = cmap.n_shapes
    cfg = SimConfig(n_envs=1, n_cops=cmap.n_cops, n_thieves=cmap.n_thieves, n_rays=rays, bbtree_gate=2)
    L, h, rdx, rdy = _grid(cmap, cfg)
    ocfg = SimConfig(n_envs=1, n_cops=cmap.n_cops, n_thieves=cmap.n_thieves, n_rays=rays, bbtree_gate=0 if S == 1 else 1)
    orc = OracleSim(ocfg, [cmap])
    rng = np.random.default_rng(seed)
    lo = cmap.shape_bb[:, :2].min(0) - 60; hi = cmap.shape_bb[:, 2:].max(0) + 60
    out = (C.c_int * 256)()
    checked = 0
    for trial in range(n_origins):
        if trial % 3 == 0:      # next to a wall's bb corner: grazing rays
            s = rng.integers(S)
            ax = cmap.shape_bb[s, rng.choice([0, 2])] + rng.uniform(-3, 3)
            ay = cmap.shape_bb[s, rng.choice([1, 3])] + rng.uniform(-3, 3)
        else:
            ax, ay = rng.uniform(lo, hi)
        for k in range(rays):
            bx, by = ax + rdx[k], ay + rdy[k]
            cand = np.arange(S) if S == 1 else np.nonzero(_tbb(cmap.shape_bb, ax, ay, bx, by) < 1.0)[0]
            n = L.cat_grid_lookup_host(h, float(ax), float(ay), k, out, 256)
            row = set(out[:n])
            for s in cand:
                if s in row:
                    continue
                sh, _, _ = orc.segment_query(0, -1, (ax, ay), (bx, by), cfg.ray_radius, los=True, walls=[int(s)])
                assert sh < 0, (cmap.name, ax, ay, k, int(s))
                checked += 1
    L.cat_grid_free_host(h)
    return checked


@pytest.mark.parametrize("name", PRESETS)
def test_tree_order_tables_list_every_wall_that_is_entered_and_hit(name):
    _check_tables(load_preset(name).compile(), n_origins=24 if name != "agh-map" else 12)


def test_tree_order_tables_on_random_maps(tmp_path):
    for seed, n in ((11, 9), (12, 40)):
        _check_tables(_random_map(tmp_path, seed, n), n_origins=16, seed=seed)


def test_tree_order_tables_of_a_single_wall_list_the_ungated_root(tmp_path):
    """D6: one wall is the root of its tree and visited ungated -- a ray whose thin segment passes beside the wall's bb but whose swept
    circle grazes the corner must find the wall on its row; and so must every ray of the sampled origins that the ungated query hits."""
    blocks = [{"type": "rect", "x": 300, "y": 300, "w": 100, "h": 100}]
    agents = [{"type": "cop", "x": 200, "y": 298.4}, {"type": "thief", "x": 100, "y": 100}]
    f = tmp_path / "one.json"
    f.write_text(json.dumps({"window": {"w_px": 1280, "h_px": 800}, "canvas": {"w": 1280, "h": 800},
                             "objects": {"blocks": blocks}, "agents": agents}))
    cmap = Map(f).compile()
    cfg = SimConfig(n_envs=1, n_cops=1, n_thieves=1, n_rays=8, bbtree_gate=2)
    L, h, _, _ = _grid(cmap, cfg)
    out = (C.c_int * 8)()
    n = L.cat_grid_lookup_host(h, 200.0, 298.4, 0, out, 8)
    assert list(out[:n]) == [0]
    L.cat_grid_free_host(h)
    _check_tables(cmap, n_origins=30, rays=16)


def test_query_order_option_is_checked_before_any_device():
    from as_cops_and_thieves_amd.environments import BaseEnv, SimpleEnv, VecCopsEnv, gate_mode
    assert gate_mode(True, "index") == 1 and gate_mode(False, "index") == 0 and gate_mode(True, "chipmunk") == 2
    m = load_preset("labyrinth")
    for make in (lambda **kw: BaseEnv(m, **kw), lambda **kw: SimpleEnv(m, **kw), lambda **kw: VecCopsEnv(m, 4, **kw)):
        with pytest.raises(ValueError, match="bbtree_gate"):
            make(query_order="chipmunk", bbtree_gate=False)
        with pytest.raises(ValueError, match="query_order"):
            make(query_order="bbtree")
    assert SimConfig(bbtree_gate=2).bbtree_gate == 2


def test_cli_flags_offer_the_query_order():
    import subprocess
    import sys
    from pathlib import Path
    for mod in ("as_cops_and_thieves_amd.driver", "as_cops_and_thieves_amd.selfplay.self_play"):
        res = subprocess.run([sys.executable, "-m", mod, "--help"], capture_output=True, text=True, timeout=120,
                             cwd=Path(__file__).resolve().parents[1])
        assert res.returncode == 0 and "--query-order" in res.stdout and "chipmunk" in res.stdout, (mod, res.stderr[-500:])


def test_cat_create_refuses_a_gate_mode_above_two():
    """The configuration is checked before the device: no GPU needed."""
    L = _lib()
    cmap = load_preset("labyrinth").compile()
    cfg = SimConfig(n_envs=4, n_rays=16, bbtree_gate=3)
    c = nat.CatConfig()
    for n in C_FIELDS_I32 + C_FIELDS_F64:
        setattr(c, n, getattr(cfg, n))
    dx, dy = tables.ray_table(cfg.sensor)
    lut = np.zeros(32768, np.float32)
    t = nat.CatTables(dx.ctypes.data, dy.ctypes.data, lut.ctypes.data, lut.ctypes.data)
    blob = cmap.to_blob()
    arr = (C.c_char_p * 1)(blob)
    sizes = (C.c_size_t * 1)(len(blob))
    h = C.c_void_p()
    assert L.cat_create(C.byref(c), C.byref(t), arr, sizes, 1, None, 0, C.byref(h)) == -1
    assert b"bbtree_gate=3" in L.cat_last_error(None)
