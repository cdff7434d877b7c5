"""The radius tests without the square root on the device (csrc/cat_sim_radius.h; termination_captured, agent_setup).

selftest ops 4 and 5 evaluate, for a squared distance x, the old predicate with the device's own square root (bit 0) and the threshold
compare the kernels now run (bit 1): for every double within 64 ulps either side of the threshold, for the radii of
tests/test_radius_thresholds_host.py, the two bits must be equal and equal to NumPy's.  Then the scripted scenario of tests/radius_cases.py --
a cop - thief pair exactly at, one ulp of the squared distance inside and one outside the capture radius, a pair of agents likewise at the
"origin inside the circle" distance -- runs one tick through the one-tick launch and through a resident launch, bit for bit against the oracle."""
import numpy as np
import pytest

from tests import radius_cases as rc
from tests.test_radius_thresholds_host import RADII, around, old_capture, old_near, thresholds
from tests.util import assert_outputs_equal, assert_state_equal, to_np

pytestmark = pytest.mark.gpu


def _selftest(op, xs, params):
    import torch
    from as_cops_and_thieves_amd import _native
    a = torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")
    b = torch.tensor(params, dtype=torch.float64, device="cuda:0")
    out = torch.empty_like(a)
    assert _native.lib().cat_selftest_arith(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), 0, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def test_device_predicates_agree_around_the_thresholds():
    for term, agent_r, ray_r in RADII:
        X, E = thresholds(term, agent_r, ray_r)
        far = np.array([0.0, 1e-300, 0.25 * term * term, 4.0 * term * term, 1e300, np.inf, np.nan])
        xs = np.concatenate([around(X), around(term * term), far])
        got = _selftest(4, xs, [term, X])
        assert np.array_equal(got & 1, got >> 1) and np.array_equal((got & 1).astype(bool), old_capture(xs, term)), (term, X)
        xs = np.concatenate([around(E), around((agent_r + ray_r) ** 2), far])
        got = _selftest(5, xs, [agent_r, ray_r, E])
        assert np.array_equal(got & 1, got >> 1) and np.array_equal((got & 1).astype(bool), old_near(xs, agent_r, ray_r)), (agent_r, ray_r, E)


def _sim(sc, debug_hit_shape):
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    gpu = CatSim(sc.cfg, [sc.cmap], device="cuda:0", debug_hit_shape=debug_hit_shape)
    g = gpu.reset(positions=torch.from_numpy(sc.start))
    torch.cuda.synchronize()
    keys = rc.OBS_KEYS if debug_hit_shape else tuple(k for k in rc.OBS_KEYS if k != "hit_shape")
    assert_outputs_equal(to_np(g), sc.reset_out, keys=keys, ctx="reset")
    gpu.set_state(**sc.placed)
    return gpu


def test_one_tick_on_the_thresholds_equals_the_oracle():
    import torch
    sc = rc.scenario()
    sc.check()
    gpu = _sim(sc, True)
    assert gpu.one_tick_kernel == "step_kernel_pooled"
    g = gpu.step(torch.from_numpy(sc.actions[0]).to("cuda:0"))
    torch.cuda.synchronize()
    assert_outputs_equal(to_np(g), sc.out, ctx="tick on the thresholds")
    assert_state_equal(to_np(gpu.get_state()), sc.state, ctx="tick on the thresholds")
    assert gpu.device_errors() == 0
    gpu.close()


def test_one_resident_tick_on_the_thresholds_equals_the_oracle():
    import torch
    sc = rc.scenario()
    gpu = _sim(sc, False)
    assert gpu.rollout_kernel == "rollout_kernel_pooled"
    rows = to_np(gpu.rollout_fused(1, torch.from_numpy(sc.actions).to("cuda:0"), tick=0, auto_reset=False))
    torch.cuda.synchronize()
    keys = tuple(k for k in rc.OBS_KEYS if k != "hit_shape") + ("reward", "terminated", "truncated", "winner")
    assert_outputs_equal({k: v[0] for k, v in rows.items()}, sc.out, keys=keys, ctx="resident tick on the thresholds")
    assert_state_equal(to_np(gpu.get_state()), sc.state, ctx="resident tick on the thresholds")
    assert gpu.device_errors() == 0
    gpu.close()
