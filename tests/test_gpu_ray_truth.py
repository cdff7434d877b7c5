"""GPU: the HIP env core (through the C ABI, tests/gpu_sim.py) against the geometric truth of tests/ray_truth.py -- not through
the oracle.  The same truth, the same clear rule, the same cap on excluded rays and zero mismatches as tests/test_ray_truth_host.py,
in every form of the ray fan cat_create can pick or be forced into, under each gate mode and through each stepping entry; the
shapes are the smallest that reach each path (5 - 12 envs).  The oracle only samples the injected start positions."""
import pytest

from tests import ray_truth_cases as rc
from tests.gpu_sim import GpuSim
from tests.ray_truth_cases import FEW_SLOTS, FIVE_MAPS, OTHERS, TREE_ORDER, Case

pytestmark = pytest.mark.gpu

LABYRINTH = FIVE_MAPS[0]
# what cat_create picks for these rosters by itself (tests/test_gpu_parity.py::test_default_choice_of_the_scheduler_per_entry)
DEFAULT_KERNEL = {"labyrinth": "step_kernel_pooled", "lbirinth": "step_kernel", "grandbyrinth": "step_kernel", "agh-map": "step_kernel"}


def _expect(one_tick=None, chunks=None):
    def check(gpu):
        if one_tick is not None:
            assert gpu.sim.one_tick_kernel == one_tick, gpu.sim.one_tick_kernel
        if chunks is not None:
            assert (gpu.sim.chunks_per_unit(True), gpu.sim.chunks_per_unit(False)) == chunks
    return check


@pytest.mark.parametrize("case", FIVE_MAPS, ids=str)
def test_default_form_on_the_five_maps(case):
    rc.reset_and_tick_case(GpuSim, case, check_kernel=_expect(DEFAULT_KERNEL.get(case.map)))


FORCED = [("chunk form", LABYRINTH, {"CAT_FAN": "chunks"}, _expect("step_kernel")),
          ("unit form", LABYRINTH, {"CAT_POOL": "0"}, _expect("step_kernel")),
          ("pooled form", FIVE_MAPS[1], {"CAT_POOL": "1"}, _expect("step_kernel_pooled")),
          ("generic kernel", LABYRINTH, {"CAT_GENERIC_KERNEL": "1"}, _expect()),
          ("group form at 130 rays", OTHERS[2], {}, _expect()),
          ("partly filled workgroup", FEW_SLOTS, {"CAT_POOL": "1"}, _expect("step_kernel_pooled")),
          ("three chunks of a slot in one unit", FIVE_MAPS[4], {"CAT_SLOT_CHUNKS": "3", "CAT_SLOT_CHUNKS_TICK": "3"}, _expect(chunks=(3, 3)))]


@pytest.mark.parametrize("what,case,switches,check", FORCED, ids=[f[0] for f in FORCED])
def test_forced_forms_of_the_ray_fan(what, case, switches, check, monkeypatch):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    rc.reset_and_tick_case(GpuSim, case, check_kernel=check, tag=what)


@pytest.mark.parametrize("case", TREE_ORDER + OTHERS[:2], ids=str)
def test_tree_order_no_gate_and_random_polygons(case, tmp_path):
    """``bbtree_gate = 2`` (the walls in the order of Chipmunk's static tree: the chunk form carries it), ``bbtree_gate = 0`` (every
    shape visited) and a map of slanted, touching and overlapping blocks, against the one truth that serves every visiting order."""
    rc.reset_and_tick_case(GpuSim, case, tmp_path, check_kernel=_expect("step_kernel" if case.gate == 2 else None))


def test_fused_step_at_a_tick_where_slots_end():
    rc.fused_step_case(GpuSim, Case("labyrinth", envs=8, max_steps=12, seed=4, label="labyrinth step_fused + respawn"))


def test_first_row_of_a_four_tick_resident_launch():
    rc.rollout_case(GpuSim, Case("labyrinth", envs=8, seed=5, label="labyrinth rollout_fused(4)"))


@pytest.mark.parametrize("name,cops,thieves", [("labyrinth", 2, 1), ("lbirinth", 2, 1)])
def test_captures_on_injected_pairs(name, cops, thieves):
    rc.capture_injection_case(GpuSim, name, cops, thieves)


@pytest.mark.parametrize("name,cops,thieves,envs", [("labyrinth", 2, 1, 12), ("grandbyrinth", 3, 2, 12), ("lbirinth", 2, 1, 64)])
def test_spawns_satisfy_the_spawn_rule(name, cops, thieves, envs):
    checked, _ = rc.spawn_case(GpuSim, name, cops, thieves, envs)
    assert checked == 2 * envs * (cops + thieves)
