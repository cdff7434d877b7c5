"""The DEVICE build of reward_arith_f16 (csrc/cat_sim_reward.h) over every float16 distance and both roles, one small launch
(cat_debug_reward_table), against the tables the handle was created with: equal bit for bit at and below ``reward_arith_max``, the index up to
which the host build equals both tables (cat_reward_arith_max).  (The host build and the scan that finds the index: tests/test_reward_arith_host.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_device_arithmetic_equals_the_tables_up_to_reward_arith_max():
    import torch
    from as_cops_and_thieves_amd import tables
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.sim import CatSim
    sim = CatSim(SimConfig(n_envs=4, n_rays=64, seed=1), [load_preset("squarinth").compile()], device="cuda:0")
    m = sim._L.cat_reward_arith_max(sim._h)
    sensor = sim.cfg.sensor
    bound = int(np.array([sensor.ray_length + sensor.ray_radius]).astype(np.float16).view(np.uint16)[0])
    print("reward_arith_max", m, "furthest sighting", bound)
    assert m >= bound and m >= 0x7C00       # every finite distance and +inf
    out = torch.full((2, 32768), float("nan"), dtype=torch.float32, device="cuda:0")
    assert sim._L.cat_debug_reward_table(sim._h, out.data_ptr(), sim._stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    for role, lut in ((0, tables.cop_reward_lut()), (1, tables.thief_reward_lut())):
        bad = np.nonzero(got[role, :m + 1] != lut[:m + 1].view(np.uint32))[0]
        assert len(bad) == 0, (role, bad[:16])
    assert sim.device_errors() == 0
    sim.close()
