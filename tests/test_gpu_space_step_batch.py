"""Space.step on the GPU against the oracle, bit for bit, on scripted scenarios (tests/space_step_cases.py) that mix contact slots and
contact-free slots in one workgroup from tick 0 and hold every shape of contact list the solver distinguishes: two wall contacts on one
body, wall contacts on several bodies of an env, agent pairs, cache entries that age and expire while nothing touches.

labyrinth 2v1 at 64 rays runs the pooled kernels (their per-slot Space.step beside the ray rounds; a pass that batched the contact-free steps of a
workgroup was built against these cases, measured slower and left out: DESIGN 4.9); squarinth 1v1 at 90 rays and grandbyrinth 3v2 run what cat_create
picks for them.  All of them solve wall-only contact lists in registers, lane = agent (solve_walls_reg), and every other list in the list-order
loop of physics_env.  Each case goes through the
one-tick entry (state and outputs after every tick) and through one resident launch (every tick's outputs, the state after the last)."""
import numpy as np
import pytest

from tests import space_step_cases as cases
from tests.util import assert_outputs_equal, assert_state_equal, to_np

pytestmark = pytest.mark.gpu


def _sim(tr, debug_hit_shape):
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    gpu = CatSim(tr.cfg, [tr.cmap], device="cuda:0", debug_hit_shape=debug_hit_shape)
    g = gpu.reset(positions=torch.from_numpy(tr.start))
    torch.cuda.synchronize()
    keys = cases.OBS_KEYS if debug_hit_shape else tuple(k for k in cases.OBS_KEYS if k != "hit_shape")
    assert_outputs_equal(to_np(g), tr.reset_out, keys=keys, ctx="reset")
    gpu.set_state(pos=tr.placed)
    return gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_one_tick_launches_equal_the_oracle_at_every_tick(name, monkeypatch):
    """(coverage counts of the cases: tests/test_space_step_host.py)"""
    import torch
    tr = cases.trace(name)
    cases.check_coverage(tr.coverage, tr.min_over_bound)
    if tr.case["pool"] is not None:
        monkeypatch.setenv("CAT_POOL", tr.case["pool"])
    gpu = _sim(tr, True)
    if tr.case["pool"] == "1":
        assert gpu.one_tick_kernel == "step_kernel_pooled"
    acts = torch.from_numpy(tr.actions).to("cuda:0")
    for t in range(len(tr.actions)):
        g = gpu.step(acts[t])
        torch.cuda.synchronize()
        assert_outputs_equal(to_np(g), tr.outs[t], ctx=f"{name} tick {t}")
        assert_state_equal(to_np(gpu.get_state()), tr.states[t], ctx=f"{name} tick {t}")
    assert gpu.device_errors() == 0
    gpu.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_one_resident_launch_equals_the_oracle(name, monkeypatch):
    import torch
    tr = cases.trace(name)
    cases.check_coverage(tr.coverage, tr.min_over_bound)
    if tr.case["pool"] is not None:
        monkeypatch.setenv("CAT_POOL", tr.case["pool"])
    gpu = _sim(tr, False)
    if tr.case["pool"] == "1":
        assert gpu.rollout_kernel == "rollout_kernel_pooled"
    T = len(tr.actions)
    rows = to_np(gpu.rollout_fused(T, torch.from_numpy(tr.actions).to("cuda:0"), tick=0, auto_reset=False))
    torch.cuda.synchronize()
    keys = tuple(k for k in cases.OBS_KEYS if k != "hit_shape") + ("reward", "terminated", "truncated", "winner")
    for t in range(T):
        assert_outputs_equal({k: v[t] for k, v in rows.items()}, tr.outs[t], keys=keys, ctx=f"{name} resident tick {t}")
    assert_state_equal(to_np(gpu.get_state()), tr.states[-1], ctx=f"{name} resident launch")
    assert gpu.device_errors() == 0
    gpu.close()
