"""GPU: ``cat_render_nav_spawn`` against ``navigation.spawn_step`` -- on synthetic buffers, through ``VecCopsEnv`` tick by tick against an env
driven by hand with the definition's outputs, inside ``MAPPOTrainer``'s rollout (eager, captured and replayed), in
``evaluate_by_separation`` and in a short training run.  Every step runs in a process of its own under its own time limit
(``tests/curriculum_steps.py``); after a step that ended in a fault, an abort or a time-out nothing more is started on the GPU: the
remaining tests fail without running.  A missing symbol or attribute fails the step that needs it."""
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
        res = subprocess.run([sys.executable, "-m", "tests.curriculum_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_the_kernel_equals_the_definition_on_synthetic_buffers():
    """N in {1, 63, 257} (one wave, a partial last workgroup, more than one workgroup: four slots to a workgroup); A = 3 as 2v1 and as 1v2
    (a second thief: the reachability rule) and A = 5 as 3v2; two maps of different sizes through slot_map; mixed masks; bands valid, off,
    lo < 1, lo > hi and valid but empty; the draws 0, 0x3F7FFFFF and one whose fp32 product rounds up to the next rank; the hand-derived
    rows of tests/curriculum_cases.py first.  f64 bits of positions and bytes of placed between guard bands; unwritten rows keep their
    pre-fill.  Bad arguments are refused and write nothing."""
    run_step("synthetic", 120)


def test_the_env_respawns_by_the_definition_and_keeps_the_terminal_tick():
    """Squarinth 2v1, 64 rays, 256 envs, max_step_count 8, 24 random ticks, band (2, 6), the draws passed in: the env with the spawner
    against one driven by hand (the same actions, then ``reset`` with the definition's mask and positions) -- every output buffer and
    ``get_env_state()`` bit-equal after every tick; terminal rows occur; their reward, flags, winner and final_positions equal a clone taken
    before a ``respawn`` by hand; ``placed.sum()`` equals the terminal rows (no fallback on this map and band).  The same with ``repeat=3``.
    ``rollout_random`` refuses while a spawner is attached; ``reset`` places the banded slots."""
    run_step("env", 180)


def test_the_trainer_respawns_inside_its_rollout_eager_captured_and_replayed():
    """64 envs, horizon 16, bptt 16, max_step_count 12, three collects without an update: the rollout buffers of a ``graph_rollout=False``
    trainer and of one that captures and replays are bit-equal; ``set_band(8, 12)`` between two replays shows in the separations of the
    slots that have just respawned, without a recapture; off, ``param_digest`` and the buffers equal a trainer built without the field."""
    run_step("trainer", 300)


def test_evaluate_by_separation_reports_per_band_and_detaches_its_spawner():
    run_step("separation_eval", 180)


def test_a_short_training_run_with_the_curriculum_stays_finite_and_reports_it():
    run_step("train", 180)
