"""GPU: Space.step of the HIP env core (through the C ABI, tests/gpu_sim.py) against the mechanical truth of tests/step_truth.py --
not through the oracle, which only produced the action tapes on the CPU.  Every tape of tests/step_truth_cases.py is replayed one
tick per launch with ``get_state`` after every tick, and every tick is held against the truth with the same clear rule, cap and
tolerances as tests/test_step_truth_host.py and zero contact-set differences: through ``cat_step`` and through
``cat_step_fused(auto_reset=0)``, with respawns between the ticks (``auto_reset=1``), in the forced forms of the kernel, and on the
injected states of a body that leaves a re-found wall.  Resident launches and ``cat_step_repeat`` are held bit-equal to one-tick
stepping elsewhere (tests/test_gpu_rollout_resident.py, tests/test_gpu_step_repeat.py)."""
import pytest

from tests import step_truth_cases as stc
from tests.gpu_sim import GpuSim

pytestmark = pytest.mark.gpu

KERNEL_OF_POOL = {"1": "step_kernel_pooled", "0": "step_kernel"}


def _expect(one_tick=None):
    def check(gpu):
        if one_tick is not None:
            assert gpu.sim.one_tick_kernel == one_tick, gpu.sim.one_tick_kernel
    return check


def _run(name, monkeypatch, entry, switches=None, one_tick=None, tag="", **kw):
    """A tape in the form its case names (the two labyrinth tapes are one tape under CAT_POOL=1 and CAT_POOL=0, with the kernel
    asserted; the others run what cat_create picks), or under the given switches."""
    pool = stc.trace(name).case["pool"]
    if switches is None:
        switches, one_tick = ({} if pool is None else {"CAT_POOL": pool}), KERNEL_OF_POOL.get(pool)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    return stc.run_case(GpuSim, name, entry=entry, check_kernel=_expect(one_tick), tag=tag or entry, **kw)


@pytest.mark.parametrize("name", stc.CASES)
def test_cat_step_on_every_tape(name, monkeypatch):
    s = _run(name, monkeypatch, "step", tag="cat_step")
    stc.check_least(name, s["counts"])


@pytest.mark.parametrize("name", stc.CASES)
def test_cat_step_fused_without_auto_reset_on_every_tape(name, monkeypatch):
    s = _run(name, monkeypatch, "fused", tag="cat_step_fused(auto_reset=0)")
    stc.check_least(name, s["counts"])


def test_cat_step_fused_with_auto_reset_leaves_out_the_respawned_slot_ticks(monkeypatch):
    s = _run("labyrinth_2v1_mixed", monkeypatch, "fused", auto_reset=True, tag="cat_step_fused(auto_reset=1)")
    assert not s["kept"].all() and s["kept"].mean() > 0.9, s["kept"].mean()
    assert s["counts"]["single"] >= 500 and s["counts"]["multi"] >= 20, s["counts"]


FORCED = [("generic kernel", "labyrinth_2v1_mixed", {"CAT_GENERIC_KERNEL": "1"}, None),
          ("generic kernel on slanted polygons", "random_12_2v1", {"CAT_GENERIC_KERNEL": "1"}, None),
          ("partly filled workgroup", "bounce_labyrinth_2v1", {"CAT_POOL": "1"}, "step_kernel_pooled")]


@pytest.mark.parametrize("what,name,switches,one_tick", FORCED, ids=[f[0] for f in FORCED])
def test_forced_forms_of_the_step(what, name, switches, one_tick, monkeypatch):
    s = _run(name, monkeypatch, "step", switches, one_tick, tag=what)
    stc.check_least(name, s["counts"])


def test_a_body_that_leaves_a_refound_wall_is_held_by_the_stale_impulse():
    stc.stale_leave_case(GpuSim)
