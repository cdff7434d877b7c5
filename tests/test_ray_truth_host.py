"""CPU: the oracle against the geometric truth of tests/ray_truth.py.

Every other env-core test compares the HIP kernels with oracle/cat_oracle.c, which restates Chipmunk's algorithm and was written
beside the kernels: a misreading the two share (an edge range, a normal's sign, the radius on the wrong side, '<' for '<=') would
pass them all.  Here the oracle's ray fan, capture test and spawn rule are held against answers that follow from the geometry
alone; tests/test_gpu_ray_truth.py holds the HIP library against the same answers without going through the oracle."""
import ast
from pathlib import Path

import numpy as np
import pytest

from tests import ray_truth as rt
from tests import ray_truth_cases as rc
from tests.ray_truth_cases import Case

from tests.ray_truth_cases import FIVE_MAPS, OTHERS, TREE_ORDER


@pytest.fixture
def tree_order():
    """The oracle's wall queries descend Chipmunk's static tree (what ``bbtree_gate = 2`` means to the library) while a test runs."""
    from oracle.cat_oracle import lib
    lib().cato_set_index_order(2)
    yield
    lib().cato_set_index_order(1)


def test_the_truth_imports_neither_the_oracle_nor_the_product():
    tree = ast.parse((Path(__file__).resolve().parent / "ray_truth.py").read_text())
    seen = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            seen |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "relative import"
            seen.add((node.module or "").split(".")[0])
        elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in ("__import__", "import_module"):
            raise AssertionError("dynamic import")
    assert seen <= {"__future__", "json", "pathlib", "numpy"}, seen


def test_hull_distance_and_first_contact_on_hand_computed_cases():
    """The truth's own primitives on a 3-4-5 corner and a unit square: answers a reader can check on paper."""
    sq = rt.gift_wrap([(0, 0), (4, 0), (4, 4), (0, 4), (2, 0), (4, 4), (2, 2)])          # an edge point, a repeat, an inner point
    assert {tuple(v) for v in sq.tolist()} == {(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0)}
    d, c = rt.hull_distance(sq, (7.0, 8.0))
    assert d == 5.0 and c.tolist() == [4.0, 4.0]                                           # the corner, 3-4-5 away
    assert rt.hull_distance(sq, (1.0, 2.0))[0] == 0.0 and rt.hull_distance(sq, (-2.0, 1.0))[0] == 2.0
    # towards the face x = 4 from the right, rho = 2: the centre stops at x = 6, a tenth of the way along a 40 px segment from x = 10
    a, m = rt.wall_alpha(sq, 2.0, (10.0, 2.0), (-40.0, 0.0))
    assert a[0] == pytest.approx(0.1, abs=1e-15) and not m[0]
    # 1.2 above the corner (4, 4): past the face's extent, on the corner circle x = 4 + sqrt(4 - 1.44) = 5.6
    a, m = rt.wall_alpha(sq, 2.0, (10.0, 5.2), (-40.0, 0.0))
    assert a[0] == pytest.approx((10.0 - 5.6) / 40.0, abs=1e-15) and not m[0]
    a, m = rt.wall_alpha(sq, 2.0, (10.0, 6.5), (-40.0, 0.0))                               # 2.5 above: passes
    assert a[0] == np.inf and not m[0]
    a, m = rt.wall_alpha(sq, 2.0, (5.0, 2.0), (40.0, 0.0))                                 # starts within rho, pointing away: alpha 0
    assert a[0] == 0.0
    assert rt.segment_hull_distance(sq, (-3.0, 7.0), (7.0, -3.0))[0] == 0.0                # crosses without an end inside
    assert rt.segment_hull_distance(sq, (5.0, 8.0), (8.0, 5.0))[0] == pytest.approx(np.hypot(2.5, 2.5), abs=1e-15)
    assert rt.box_entry([0, 0, 4, 4], np.array([[-4.0, 2.0]]), np.array([[16.0, 0.0]]))[0] == 0.25


@pytest.mark.parametrize("case", FIVE_MAPS, ids=str)
def test_oracle_rays_and_captures_on_the_five_maps(case):
    rc.reset_and_tick_case(rc.oracle_sim, case)


@pytest.mark.parametrize("case", TREE_ORDER, ids=str)
def test_oracle_rays_in_tree_order(tree_order, case):
    """One truth serves both visiting orders: on a clear ray the winner is visited, and wins, under any order."""
    rc.reset_and_tick_case(rc.oracle_sim, case)


@pytest.mark.parametrize("case", OTHERS, ids=str)
def test_oracle_rays_ungated_on_random_polygons_and_with_130_rays(case, tmp_path):
    rc.reset_and_tick_case(rc.oracle_sim, case, tmp_path)


def test_oracle_rays_of_a_respawned_slot_and_of_a_four_tick_rollout():
    """The scenarios of the library's fused entries, on the oracle's step + masked reset (the GPU test runs them on the entries)."""
    rc.fused_step_case(rc.oracle_sim, Case("labyrinth", envs=8, max_steps=12, seed=4, label="labyrinth step + respawn"))
    rc.rollout_case(rc.oracle_sim, Case("labyrinth", envs=8, seed=5, label="labyrinth four ticks"))


@pytest.mark.parametrize("name,cops,thieves", [("labyrinth", 2, 1), ("lbirinth", 2, 1)])
def test_oracle_captures_on_injected_pairs(name, cops, thieves):
    """Pairs inside the radius in the open, inside it with a wall between them, and just outside it.  No wall of the labyrinth is
    thinner than the radius (its blocks are 36 px and more), so there the wall between is a block's corner; the lbirinth's 5 px walls
    are straddled."""
    rc.capture_injection_case(rc.oracle_sim, name, cops, thieves)


@pytest.mark.parametrize("name,cops,thieves,envs", [("labyrinth", 2, 1, 12), ("grandbyrinth", 3, 2, 12), ("lbirinth", 2, 1, 64)])
def test_oracle_spawns_satisfy_the_spawn_rule(name, cops, thieves, envs):
    checked, moved = rc.spawn_case(rc.oracle_sim, name, cops, thieves, envs)
    assert checked == 2 * envs * (cops + thieves)


# measured on this test's own run: a truth with ray radius 0.9 disagrees with the oracle on SENSITIVITY_MEASURED of the clear
# distances; the floor is half of that
SENSITIVITY_MEASURED = 0.169   # 388 of 2294 clear rays
SENSITIVITY_FLOOR = SENSITIVITY_MEASURED / 2


def test_a_tenth_of_a_pixel_in_the_ray_radius_is_seen():
    """The check has teeth: the same comparison against a truth whose swept disc is 0.1 px too small must fail on a clear share of
    the distances (and the right radius on none)."""
    case = Case("labyrinth", envs=12)
    cmap, cfg = rc.compiled_case_map(case), rc.config_for(case)
    sim, truth = rc.oracle_sim(cfg, [cmap]), rc.truth_for(cmap, cfg)
    pos = rc.free_positions(rc.oracle_sim(cfg, [cmap]), cmap, np.random.default_rng(case.seed), spread=60)
    out = sim.reset(positions=pos)
    st = sim.get_state()
    right = truth.observe(st["pos"], st["tc"], st["leaf_bb"])
    wrong = truth.observe(st["pos"], st["tc"], st["leaf_bb"], ray_radius=0.9)
    seen = right["clear"]
    assert not (seen & (out["obs_distance"] != right["obs_distance"])).any()
    share = float((seen & (out["obs_distance"] != wrong["obs_distance"])).sum()) / float(seen.sum())
    line = f"ray-truth sensitivity: ray radius 0.9 for 1.0 changes {100 * share:.1f} % of {int(seen.sum())} clear distances (labyrinth, reset)"
    rc.REPORT.append(line)
    print(line)
    assert share >= SENSITIVITY_FLOOR > 0.05
