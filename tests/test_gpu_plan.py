"""On the device the sim is built from the plan: what cat_create prints under CAT_VERBOSE=1 is, byte for byte, what cat_plan_describe_host returns for
the same arguments without a device; the kernel names and chunks per unit the handle reports agree with it; and the sim so created resets and steps
without a device-side error."""
import os
import re
import tempfile

import pytest

from tests import plan_cases as pc
from tests.plan_cases import PlanCase

pytestmark = pytest.mark.gpu

SMALL = {
    "labyrinth": PlanCase(("labyrinth",), 2, 1, 64, 64),
    "agh": PlanCase(("agh-map",), 2, 1, 64, 64),
    "labyrinth_agh_split": PlanCase(("labyrinth", "agh-map"), 2, 1, 64, 128, slots="interleave", env={"CAT_SPLIT": "1"}),
}


class _Stderr:
    """File descriptor 2 into a temporary file for a while (the library writes with fputs, not through sys.stderr)."""

    def __enter__(self):
        self._file = tempfile.TemporaryFile()
        self._saved = os.dup(2)
        os.dup2(self._file.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self._saved, 2)
        os.close(self._saved)
        self._file.seek(0)
        self.text = self._file.read().decode()
        self._file.close()


@pytest.mark.parametrize("name", list(SMALL))
def test_cat_create_builds_the_sim_its_plan_describes(name):
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    case = SMALL[name]
    maps, cfg = pc.compiled_maps(case), pc.sim_config(case)
    want = pc.describe_case(case)
    with pc.knobs(dict(case.env, CAT_VERBOSE="1")), _Stderr() as err:
        sim = CatSim(cfg, maps, slot_map_ids=case.slot_map_ids(), device="cuda:0")
    try:
        printed = "".join(ln + "\n" for ln in err.text.splitlines() if re.match(r"(sim|part\d+)\.", ln))   # (the runtime may print lines of its own)
        assert printed == want
        value = lambda key: re.findall(rf"^{re.escape(key)}=(.*)$", want, re.M)
        n_parts = int(value("sim.n_parts")[0])
        assert n_parts == (2 if name == "labyrinth_agh_split" else 1)
        assert sim.one_tick_kernel == "+".join(value(f"part{i}.one_tick_kernel")[0] for i in range(n_parts))
        assert sim.rollout_kernel == "+".join(value(f"part{i}.rollout_kernel")[0] for i in range(n_parts))
        last = f"part{n_parts - 1}"
        spans = lambda key: max(int(v) for v in re.findall(rf"^{last}\.map\d+\.{key}=(\d+)$", want, re.M))
        assert sim.chunks_per_unit(True) == spans("span") and sim.chunks_per_unit(False) == spans("span_tick")
        sim.reset()
        sim.step(sim.random_actions(0))
        torch.cuda.synchronize()
        assert sim.device_errors() == 0
    finally:
        sim.close()
