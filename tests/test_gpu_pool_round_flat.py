"""The pooled kernels (step_kernel_pooled / rollout_kernel_pooled) against the oracle, bit for bit, at the shapes of tests/pool_round_flat_cases.py:
a slot's front reserves the ring entries of up to four chunks at once (one group at 2v1 / 64 rays, two groups at 90 rays and at 3v2, the
ring of exact capacity, the generic kernels), and the round reads an agent's float16 origin from the slot's env area.  Every case goes through
the one-tick entry, checked after every tick, and through one resident launch of the same eight ticks."""
import pytest

from tests import pool_round_flat_cases as cases
from tests.util import assert_outputs_equal, assert_state_equal, to_np

pytestmark = pytest.mark.gpu


def _sim(tr, debug_hit_shape, monkeypatch):
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    for k, v in tr.case["env"].items():
        monkeypatch.setenv(k, v)
    gpu = CatSim(tr.cfg, [tr.cmap], device="cuda:0", debug_hit_shape=debug_hit_shape)
    g = gpu.reset(positions=torch.from_numpy(tr.start))
    torch.cuda.synchronize()
    keys = cases.OBS_KEYS if debug_hit_shape else tuple(k for k in cases.OBS_KEYS if k != "hit_shape")
    assert_outputs_equal(to_np(g), tr.reset_out, keys=keys, ctx="reset")
    return gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_one_tick_launches_equal_the_oracle_at_every_tick(name, monkeypatch):
    import torch
    tr = cases.trace(name)
    tr.check()
    gpu = _sim(tr, True, monkeypatch)
    assert gpu.one_tick_kernel == "step_kernel_pooled"
    acts = torch.from_numpy(tr.actions).to("cuda:0")
    for t in range(cases.TICKS):
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
    gpu = _sim(tr, False, monkeypatch)
    assert gpu.rollout_kernel == "rollout_kernel_pooled"
    rows = to_np(gpu.rollout_fused(cases.TICKS, torch.from_numpy(tr.actions).to("cuda:0"), tick=0, auto_reset=False))
    torch.cuda.synchronize()
    keys = tuple(k for k in cases.OBS_KEYS if k != "hit_shape") + ("reward", "terminated", "truncated", "winner")
    for t in range(cases.TICKS):
        assert_outputs_equal({k: v[t] for k, v in rows.items()}, tr.outs[t], keys=keys, ctx=f"{name} resident tick {t}")
    assert_state_equal(to_np(gpu.get_state()), tr.states[-1], ctx=f"{name} resident launch")
    assert gpu.device_errors() == 0
    gpu.close()
