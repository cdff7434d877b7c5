"""GPU: ``cat_render_nav_shape`` against ``navigation.shaping_step`` -- on synthetic buffers, on the env's own buffers tick by tick (with the
telescoping identity as an independent truth), and inside ``MAPPOTrainer``'s rollout, eager and captured.  Every step runs in a process of
its own under its own time limit (``tests/shaping_steps.py``); after a step that ended in a fault, an abort or a time-out nothing more is
started on the GPU: the remaining tests fail without running.  A missing symbol fails the step that needs it."""
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
        res = subprocess.run([sys.executable, "-m", "tests.shaping_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_the_kernel_equals_the_definition_on_synthetic_buffers():
    """N in {1, 63, 257} (partial waves, a partial workgroup, more than one workgroup); A = 3 with G = 3 and A = 5 with G = 2 (agents 2 and
    3); two maps through slot_map; reward and shaping rows of a [G, T, N] buffer (row stride T * N) between guard bands; shaping_out given
    and NULL; three ticks chained through hops_prev; prime.  The rows are the hand-derived ones of tests/shaping_cases.py plus random ones
    with every special position.  u32 bits of reward_out and shaping_out, ints of hops_prev.  Bad arguments are refused."""
    run_step("synthetic", 120)


def test_the_kernel_equals_the_definition_on_an_env_that_times_out():
    """Squarinth 2v1, 64 rays, 256 envs, max_step_count 8, 24 random ticks: timeout rows are certain (and asserted)."""
    run_step("env_timeout", 120)


def test_the_kernel_equals_the_definition_and_telescopes_on_an_env_with_captures():
    """Squarinth 2v1, 64 rays, 256 envs, max_step_count 400, cops "pursue", thieves random, 200 ticks: capture rows occur; kernel ==
    definition on every tick; with gamma = 1, coefficients +-2^-3 and no effective cap the shaping terms of every completed episode whose
    separations were all defined sum to phi_end - phi(d_start) exactly, and these are at least 8 and at least 90 % of the completed ones
    (measured beforehand with the definition on the oracle-backed stand-in: 1.000 on the arena field, 0.598 on the navigators' plain
    field, profiles/geodesic_shaping.txt)."""
    run_step("env_capture", 180)


def test_the_trainer_shapes_its_reward_rows_and_nothing_else_eager_and_captured():
    """64 envs, horizon 16, bptt 16, max_step_count 12, three collects without an update: off and on play the same trajectory, rew_on ==
    fp32(rew_off + shape) bit for bit, shape is not all zero, episode_stats are equal; a third trainer with graph_rollout=False gives
    bit-equal rew and shape on all three collects (eager, captured, replayed)."""
    run_step("trainer", 240)


def test_a_short_training_run_with_shaping_stays_finite_and_reports_it():
    run_step("train", 180)
