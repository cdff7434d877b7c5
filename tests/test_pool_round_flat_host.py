"""The inputs of tests/test_gpu_pool_round_flat.py hold what they are meant to: counted from the oracle's own results, rays that end on a wall, on an
agent and on nothing in every case; and by the plan (no device), the pooled kernels for both entries, with the ring and the chunk count each
case is there for."""
import pytest

from tests import plan_cases as pc
from tests import pool_round_flat_cases as cases


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_has_wall_agent_and_empty_rays(name):
    tr = cases.trace(name)
    print(name, tr.counts(), tr.situations())
    tr.check()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_runs_the_pooled_kernels(name):
    c = cases.CASES[name]
    text = pc.describe_case(pc.PlanCase((c["map"],), c["cops"], c["thieves"], c["rays"], c["n"], env=c["env"]))
    kv = dict(ln.split("=", 1) for ln in text.splitlines())
    assert kv["part0.one_tick_kernel"].startswith("step_kernel_pooled") and kv["part0.rollout_kernel"].startswith("rollout_kernel_pooled"), kv
    assert ("generic" in kv["part0.kernel_variant"]) == ("CAT_GENERIC_KERNEL" in c["env"]), kv["part0.kernel_variant"]
    exact = int(kv["part0.pool_shift"]) >= 0                 # the ring's capacity is no power of two
    two_groups = name in ("labyrinth_2v1_r90_exact_ring", "grandbyrinth_3v2_r64")
    assert exact == two_groups, kv["part0.pool_shift"]
    chunks = (c["cops"] + c["thieves"]) * ((c["rays"] + 63) // 64)
    assert (chunks > 4) == two_groups, chunks                # a second group of chunks in a slot's front
