"""GPU: ``cat_act_collect_step`` (include/cat_act.h) and ``TrainerConfig(fused_collect=True)``.  Every step runs in a process of its own under
its own time limit (``tests/collect_steps.py``); after a step that ended in a fault, an abort or a time-out nothing more is started on the GPU:
the remaining tests fail without running.

4. ratio: the figures (largest |stored log-probability - the training forward's| over the first minibatch, per-layer chain against the fused
tick) are printed by the step; see profiles/fused_collect.txt for a recorded run."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FAULT = {"step": None}


def run_step(step: str, seconds: int):
    if FAULT["step"] is not None:
        pytest.fail(f"not run: step {FAULT['step']!r} ended in a fault or a time-out; nothing more is started on the GPU")
    try:
        res = subprocess.run([sys.executable, "-m", "tests.collect_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_collect_kernel_equals_act_step_and_rollout_pack_bit_for_bit():
    run_step("kernel", 180)


def test_fused_rollout_equals_a_from_trainer_actor_on_a_twin_env():
    run_step("rollout", 180)


def test_replayed_rollout_reads_the_updated_weights():
    run_step("graph", 240)


def test_stored_logp_is_within_twice_the_chains_gap_to_the_training_forward():
    run_step("ratio", 240)


def test_training_and_a_role_phase_run_through_the_fused_tick():
    run_step("end_to_end", 300)
