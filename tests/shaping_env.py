"""``tests/fake_env.OracleVecEnv`` with what ``GeodesicShaper`` needs of an env (test infrastructure): ``raw_outputs()`` with
``team_positions``, ``final_positions``, ``terminated`` and ``truncated`` as ``VecCopsEnv(final_positions=True)`` keeps them, and the
attributes ``NavField.from_env`` reads."""
import numpy as np
import torch

from tests.fake_env import OracleVecEnv


class ShapingOracleEnv(OracleVecEnv):
    def __init__(self, cmap, num_envs, **kw):
        super().__init__(cmap, num_envs, **kw)
        self._cfg, self._compiled = self.cfg, [cmap]
        A = len(self.possible_agents)
        self._final = torch.full((num_envs, A, 2), float("nan"), dtype=torch.float16)
        self._term = torch.zeros(num_envs, dtype=torch.uint8)
        self._trunc = torch.zeros(num_envs, dtype=torch.uint8)

    def _team(self):
        return torch.from_numpy(self.sim.out["team_positions"].view(np.float16).copy())

    def step(self, actions):
        before = self._team()                   # a terminal row's final_positions: the tick-start positions of the tick that ended it
        res = super().step(actions)
        term, trunc = res[2][self.possible_agents[0]], res[3][self.possible_agents[0]]
        self._final[term] = before[term]        # every other row is not written
        self._term, self._trunc = term.to(torch.uint8), trunc.to(torch.uint8)
        return res

    def raw_outputs(self):
        return {"team_positions": self._team(), "final_positions": self._final, "terminated": self._term, "truncated": self._trunc}
