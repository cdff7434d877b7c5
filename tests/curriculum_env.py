"""``tests/shaping_env.ShapingOracleEnv`` with what ``GeodesicSpawner`` needs of an env (test infrastructure): ``set_spawner``, the respawn
right after the tick as ``VecCopsEnv._step_sim`` has it, ``winner`` in ``raw_outputs()`` and the oracle's ``reset(mask, positions)`` as the
masked reset of the core."""
import numpy as np
import torch

from tests.shaping_env import ShapingOracleEnv


class CurriculumOracleEnv(ShapingOracleEnv):
    def __init__(self, cmap, num_envs, **kw):
        super().__init__(cmap, num_envs, **kw)
        self._spawner = None
        self._winner = torch.full((num_envs,), -1, dtype=torch.int8)

    def set_spawner(self, spawner=None):
        self._spawner = spawner

    def _spawn_reset(self, mask, positions):
        self.sim.reset(mask=mask.cpu().numpy().astype(np.uint8), positions=positions.cpu().numpy())

    def reset(self, seed=None, options=None):
        res = super().reset(seed, options)
        if self._spawner is not None:
            self._spawner.place_reset(None)
            return self._obs(), res[1]
        return res

    def step(self, actions):
        res = super().step(actions)             # the oracle's tick and its auto-reset; rewards and flags are copies of the terminal tick's
        self._winner = res[4]["winner"].to(torch.int8)
        if self._spawner is not None:
            self._spawner.respawn(self.raw_outputs())
            return (self._obs(),) + tuple(res[1:])
        return res

    def raw_outputs(self):
        return dict(super().raw_outputs(), winner=self._winner)

    def rollout_random(self, ticks, tick0=0):
        if self._spawner is not None:
            raise ValueError("rollout_random with a spawner attached: the resident launch cannot respawn between its ticks")
        raise NotImplementedError
