"""Tree order on the GPU (``bbtree_gate = 2``: the walls of every segment query visited in the depth-first order of Chipmunk's static
BBTree) against the CPU oracle in the same order (``cato_set_index_order(2)``), bit for bit: every output and the whole body state.
The discriminating half: in the same states an oracle in index order (mode 1) reports other shapes on some rays, so these runs show
the mode is really another order and not index order under another name."""
import numpy as np
import pytest

from tests.util import assert_outputs_equal, assert_state_equal, compiled, free_positions, to_np

pytestmark = pytest.mark.gpu

OBS_KEYS = ("obs_distance", "obs_type", "hit_shape", "shared_distance", "shared_type", "team_positions")
FLAG_KEYS = ("reward", "terminated", "truncated", "winner")


@pytest.fixture
def tree_order():
    """The oracle's segment queries descend Chipmunk's static tree while a test runs; index order again afterwards."""
    from oracle.cat_oracle import lib
    L = lib()
    L.cato_set_index_order(2)
    yield L
    L.cato_set_index_order(1)


def _run_tree(L, cfg, maps, slot, ticks, rng, auto_reset=True):
    """GPU (tree order) against the oracle in mode 2, every tick; each tick also stepped by an oracle in mode 1 from the same state.
    Returns the number of rays on which mode 1 and mode 2 report different shapes."""
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    from oracle.cat_oracle import OracleSim
    assert cfg.bbtree_gate == 2
    gpu = CatSim(cfg, maps, slot, device="cuda:0", debug_hit_shape=True)
    cpu, idx = OracleSim(cfg, maps, slot), OracleSim(cfg, maps, slot)
    assert gpu.one_tick_kernel == "step_kernel" and gpu.rollout_kernel == "rollout_kernel"   # tree order runs the chunk form, never pooled
    pos = free_positions(cpu, maps[0], rng) if slot is None else None
    if pos is not None:
        g = gpu.reset(positions=torch.from_numpy(pos)); c = cpu.reset(positions=pos)
    else:
        g = gpu.reset(); c = cpu.reset()
    torch.cuda.synchronize()
    assert_outputs_equal(to_np(g), c, keys=OBS_KEYS, ctx="reset")
    assert_state_equal(to_np(gpu.get_state()), cpu.get_state(), ctx="reset")
    differ = 0
    for t in range(ticks):
        a = cpu.random_actions(t)
        before = cpu.get_state()
        g = gpu.step(gpu.random_actions(t)); c = cpu.step(a)
        L.cato_set_index_order(1)
        idx.set_state(**before)
        o1 = idx.step(a)
        L.cato_set_index_order(2)
        differ += int((o1["hit_shape"] != c["hit_shape"]).sum())
        torch.cuda.synchronize()
        assert_outputs_equal(to_np(g), c, ctx=f"tick {t}")
        assert_state_equal(to_np(gpu.get_state()), cpu.get_state(), ctx=f"tick {t}")
        if auto_reset:
            done = c["terminated"].copy()
            gpu.reset_done(); cpu.reset(mask=done)
            if done.any():
                torch.cuda.synchronize()
                assert_outputs_equal(to_np(gpu.out), cpu.out, keys=OBS_KEYS, ctx=f"auto-reset {t}")
                assert_state_equal(to_np(gpu.get_state()), cpu.get_state(), ctx=f"auto-reset {t}")
    assert gpu.device_errors() == 0
    gpu.close()
    return differ


def _agh_3v2():
    """The dense map with a 3v2 roster (its preset has start positions for 2v1): two more start points in the open."""
    from as_cops_and_thieves_amd.maps import Map, bundled_map_path
    pts = [(300, 400), (300, 350), (350, 350), (400, 400), (350, 300)]
    return Map(bundled_map_path("agh-map"), roster=["cop"] * 3 + ["thief"] * 2, start_positions=pts).compile()


# index order reports another shape on 1900 - 11600 rays of each of these runs (the oracle's two modes); at least 20 are asked
@pytest.mark.parametrize("name,rays", [("squarinth", 90), ("lbirinth", 64), ("lbirinth", 90), ("grandbyrinth", 64), ("labyrinth", 64), ("agh-map", 64)])
def test_tree_order_parity(tree_order, name, rays):
    import zlib
    from as_cops_and_thieves_amd.config import SimConfig
    cfg = SimConfig(n_envs=64, n_rays=rays, max_step_count=400, seed=31, bbtree_gate=2)
    differ = _run_tree(tree_order, cfg, [compiled(name)], None, ticks=200, rng=np.random.default_rng(zlib.crc32(name.encode()) + rays))
    print(f"{name} {rays} rays: index order reports another shape on {differ} rays")
    assert differ >= 20


def test_tree_order_mixed_batch(tree_order):
    from as_cops_and_thieves_amd.config import SimConfig
    maps = [compiled(n) for n in ("agh-map", "grandbyrinth", "labyrinth", "lbirinth", "squarinth")]
    N = 75
    slot = (np.arange(N) % 5).astype(np.int32)
    cfg = SimConfig(n_envs=N, n_rays=64, max_step_count=40, seed=41, bbtree_gate=2)
    differ = _run_tree(tree_order, cfg, maps, slot, ticks=80, rng=np.random.default_rng(3))
    assert differ >= 20


def test_tree_order_three_vs_two_on_the_dense_map(tree_order):
    from as_cops_and_thieves_amd.config import SimConfig
    cfg = SimConfig(n_envs=32, n_cops=3, n_thieves=2, n_rays=64, max_step_count=60, seed=43, bbtree_gate=2)
    differ = _run_tree(tree_order, cfg, [_agh_3v2()], None, ticks=100, rng=np.random.default_rng(5))
    assert differ >= 20


def test_tree_order_resident_and_fused_entries(tree_order):
    """cat_rollout_fused (T = 64, auto-reset) and cat_step_fused in tree order, row by row against the oracle in mode 2."""
    import torch
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim
    from oracle.cat_oracle import OracleSim
    for name in ("lbirinth", "agh-map"):
        m = compiled(name)
        cfg = SimConfig(n_envs=64, n_rays=64, max_step_count=30, seed=47, bbtree_gate=2)
        gpu, cpu = CatSim(cfg, [m], device="cuda:0", debug_hit_shape=True), OracleSim(cfg, [m])
        gpu.reset(); cpu.reset()
        rows = to_np(gpu.rollout_fused(64, None, tick=0, auto_reset=True))
        torch.cuda.synchronize()
        for t in range(64):
            c = cpu.step(cpu.random_actions(t))
            flags = {k: c[k].copy() for k in FLAG_KEYS}
            cpu.reset(mask=c["terminated"].copy())
            got = {k: v[t] for k, v in rows.items()}
            assert_outputs_equal(got, cpu.out, keys=OBS_KEYS, ctx=f"{name} resident tick {t}")
            assert_outputs_equal(got, flags, keys=FLAG_KEYS, ctx=f"{name} resident tick {t}")
        assert_state_equal(to_np(gpu.get_state()), cpu.get_state(), ctx=f"{name} after the resident launch")
        for t in range(64, 104):
            g = to_np(gpu.step_fused(None, tick=t, auto_reset=True))
            c = cpu.step(cpu.random_actions(t))
            flags = {k: c[k].copy() for k in FLAG_KEYS}
            cpu.reset(mask=c["terminated"].copy())
            torch.cuda.synchronize()
            assert_outputs_equal(g, cpu.out, keys=OBS_KEYS, ctx=f"{name} fused tick {t}")
            assert_outputs_equal(g, flags, keys=FLAG_KEYS, ctx=f"{name} fused tick {t}")
            assert_state_equal(to_np(gpu.get_state()), cpu.get_state(), ctx=f"{name} fused tick {t}")
        assert int(cpu.get_state()["reset_count"].min()) >= 2
        assert gpu.device_errors() == 0
        gpu.close()


def test_tree_order_single_wall_root_is_visited_ungated(tree_order, tmp_path):
    """D6 in tree order: with one wall the tree's root is a leaf, which Chipmunk queries without the bb gate.  A ray whose swept circle
    grazes the wall's rounded corner while its thin segment passes 0.6 px outside the wall's bb: index order's gate drops it (EMPTY),
    tree order reports the wall, as the oracle does in mode 2."""
    import torch
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim
    from oracle.cat_oracle import OracleSim
    from tests.test_oracle_known_answers import make_map
    WALL, EMPTY = 0, 4
    cmap = make_map(tmp_path, [{"type": "rect", "x": 300, "y": 300, "w": 100, "h": 100}],
                    [{"type": "cop", "x": 200, "y": 298.4}, {"type": "thief", "x": 100, "y": 100}])
    pos = np.array([[[200.0, 298.4], [100.0, 100.0]]] * 4)
    got = {}
    for gate in (1, 2):
        cfg = SimConfig(n_envs=4, n_cops=1, n_thieves=1, n_rays=8, bbtree_gate=gate)
        gpu = CatSim(cfg, [cmap], device="cuda:0", debug_hit_shape=True)
        out = to_np(gpu.reset(positions=torch.from_numpy(pos)))
        torch.cuda.synchronize()
        got[gate] = out
        if gate == 2:
            assert_outputs_equal(out, OracleSim(cfg, [cmap]).reset(positions=pos), keys=OBS_KEYS, ctx="single wall, tree order")
        gpu.close()
    assert got[1]["obs_type"][0, 0, 0] == EMPTY
    assert got[2]["obs_type"][0, 0, 0] == WALL and got[2]["hit_shape"][0, 0, 0] == 0


def test_tree_order_single_wall_stepping(tree_order, tmp_path):
    """One wall, agents spawned around it and stepped: every ray and the state against the oracle in mode 2 (the ungated root on
    every query, the line-of-sight test of the captures included)."""
    from as_cops_and_thieves_amd.config import SimConfig
    from tests.test_oracle_known_answers import make_map
    cmap = make_map(tmp_path, [{"type": "rect", "x": 300, "y": 300, "w": 100, "h": 100}],
                    [{"type": "cop", "x": 200, "y": 298.4}, {"type": "cop", "x": 420, "y": 402}, {"type": "thief", "x": 298, "y": 250}],
                    window=(700, 700))
    cfg = SimConfig(n_envs=48, n_rays=64, max_step_count=50, seed=53, bbtree_gate=2)
    _run_tree(tree_order, cfg, [cmap], None, ticks=80, rng=np.random.default_rng(9))


def test_generic_kernel_span_on_three_vs_two(monkeypatch):
    """The chunks a work unit spans follow from the kernels select_kernels chose: with the generic instantiation (which does not carry
    fan_slot) every unit is one chunk, so no chunk is left untraced -- agh-map 3v2, index order, against the oracle."""
    import torch
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim
    from oracle.cat_oracle import OracleSim
    monkeypatch.setenv("CAT_GENERIC_KERNEL", "1")
    m = _agh_3v2()
    cfg = SimConfig(n_envs=32, n_cops=3, n_thieves=2, n_rays=64, max_step_count=30, seed=59)
    gpu, cpu = CatSim(cfg, [m], device="cuda:0", debug_hit_shape=True), OracleSim(cfg, [m])
    assert gpu.chunks_per_unit(True) == 1 and gpu.chunks_per_unit(False) == 1
    gpu.reset(); cpu.reset()
    for t in range(40):
        g = to_np(gpu.step_fused(None, tick=t, auto_reset=True))
        c = cpu.step(cpu.random_actions(t))
        flags = {k: c[k].copy() for k in FLAG_KEYS}
        cpu.reset(mask=c["terminated"].copy())
        torch.cuda.synchronize()
        assert_outputs_equal(g, cpu.out, keys=OBS_KEYS, ctx=f"tick {t}")
        assert_outputs_equal(g, flags, keys=FLAG_KEYS, ctx=f"tick {t}")
    rows = to_np(gpu.rollout_fused(20, None, tick=40, auto_reset=True))
    torch.cuda.synchronize()
    for t in range(20):
        c = cpu.step(cpu.random_actions(40 + t))
        cpu.reset(mask=c["terminated"].copy())
        assert_outputs_equal({k: v[t] for k, v in rows.items()}, cpu.out, keys=OBS_KEYS, ctx=f"resident tick {t}")
    assert_state_equal(to_np(gpu.get_state()), cpu.get_state(), ctx="after the resident launch")
    gpu.close()


def test_bbtree_gate_above_two_is_refused():
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim, CatSimError
    m = compiled("labyrinth")
    with pytest.raises(CatSimError, match="BAD_CONFIG|bbtree_gate"):
        CatSim(SimConfig(n_envs=4, n_rays=16, bbtree_gate=3), [m], device="cuda:0")
