"""GPU: ``cat_act_step`` (include/cat_act.h) and the fused ``PolicyActor``.  Every step runs in a process of its own under its own time
limit (``tests/act_steps.py``); after a step that ended in a fault, an abort or a time-out nothing more is started on the GPU: the
remaining tests fail without running.

3. accuracy: the figures (fp64 reference; fused kernel against the per-layer kernel chain) are printed by the step; see
profiles/act_step.txt, section 1, for a recorded run."""
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
        res = subprocess.run([sys.executable, "-m", "tests.act_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_sampling_rule_is_cat_rollout_samples_exactly():
    run_step("sampling", 420)


def test_state_semantics_are_exact():
    run_step("state", 180)


def test_accuracy_against_fp64_is_within_twice_the_chains():
    run_step("accuracy", 420)


def test_act_and_env_tick_replay_from_a_graph_bit_for_bit():
    run_step("graph", 180)


def test_watch_and_tracked_evaluation_through_the_fused_actor():
    run_step("end_to_end", 300)
