"""The OracleSim surface on top of CatSim (ctypes -> libcat_sim.so): GPU tests that hold the HIP library against known answers
or against the geometric truth drive it through this adapter, with NumPy arrays in and out."""
import numpy as np

from tests.util import to_np


class GpuSim:
    """The OracleSim surface the cases use, on top of CatSim (ctypes -> libcat_sim.so)."""

    def __init__(self, cfg, cmaps):
        import torch
        from as_cops_and_thieves_amd.sim import CatSim
        self.torch, self.cfg = torch, cfg
        self.sim = CatSim(cfg, cmaps, device="cuda:0", debug_hit_shape=True)
        self.N, self.A, self.R = self.sim.N, self.sim.A, self.sim.R

    def _out(self):
        self.torch.cuda.synchronize()
        return to_np(self.sim.out)

    def reset(self, mask=None, positions=None):
        t = self.torch
        self.sim.reset(mask=None if mask is None else t.as_tensor(np.ascontiguousarray(mask, np.uint8)),
                       positions=None if positions is None else t.as_tensor(np.ascontiguousarray(positions, np.float64)))
        return self._out()

    def step(self, actions):
        self.sim.step(self.torch.as_tensor(np.ascontiguousarray(actions, np.int32)))
        return self._out()

    def step_fused(self, actions, auto_reset=True):
        self.sim.step_fused(self.torch.as_tensor(np.ascontiguousarray(actions, np.int32)), auto_reset=auto_reset)
        return self._out()

    def rollout_fused(self, actions, auto_reset=True):
        """``actions`` [T, N, A] -> the T rows of every output."""
        a = self.torch.as_tensor(np.ascontiguousarray(actions, np.int32))
        rows = self.sim.rollout_fused(a.shape[0], a, auto_reset=auto_reset)
        self.torch.cuda.synchronize()
        return to_np(rows)

    def random_actions(self, tick):
        return self.sim.random_actions(tick).cpu().numpy()

    def get_state(self):
        return to_np(self.sim.get_state())

    def set_state(self, **arrays):
        self.sim.set_state(**arrays)

    def device_errors(self):
        return self.sim.device_errors()

    def close(self):
        self.sim.close()
