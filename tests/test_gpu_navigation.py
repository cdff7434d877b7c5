"""GPU: ``cat_render_nav_build`` against ``navigation.hops_reference``, ``cat_render_nav_step`` against ``navigation.navigate_step`` on
synthetic buffers and on an env, a captured (act, step) tick, and a ``NavigatorActor`` as a ``MAPPOTrainer`` opponent.  Every step runs in a
process of its own under its own time limit (``tests/navigation_steps.py``); after a step that ended in a fault, an abort or a time-out
nothing more is started on the GPU: the remaining tests fail without running.  A missing symbol fails the step that needs it."""
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
        res = subprocess.run([sys.executable, "-m", "tests.navigation_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_the_built_table_equals_hops_reference():
    """Whole tables, exact: the 7 x 5 mask with its pocket, 1 x 1 (free and blocked), 1 x 9, 64 x 64 (4096 cells, a seeded 30 % blocked),
    13 x 9 all free, a two-map batch (7 x 5 and 13 x 9: the offsets); the labyrinth at cell 16 on 64 seeded goal rows plus rows 0 and C - 1."""
    run_step("build", 120)


def test_the_tick_equals_navigate_step_on_synthetic_buffers():
    """N = 70 (the last workgroup is not full), A = 3 (2v1) and A = 5 (3v2), a two-map slot_map, three segments with a -1 for one navigator,
    nav_hops bound and NULL.  The generator's shares (a tenth of the rows each: invalid position, snapped, no snap, unreachable target,
    same cell, each tie-break) are asserted on the CPU first; actions and hops exact, sentinels and guard bands intact."""
    run_step("synthetic", 90)


def test_fused_actor_equals_navigate_step_on_an_env_for_200_ticks():
    """Labyrinth 2v1, 64 envs, 64 rays, cops pursue, thief flees: action for action and hop for hop, every tick; device_errors 0."""
    run_step("env", 120)


def test_a_captured_tick_replays_the_eager_loop():
    """(act, step_raw) captured once and replayed for 20 ticks from the same uniform numbers and the same initial state."""
    run_step("graph", 120)


def test_a_navigator_opponent_stays_inside_the_captured_rollout():
    """``MAPPOTrainer.set_opponent("thief", NavigatorActor(...))`` on squarinth at 64 envs, 16-tick rollouts with ``graph_rollout=True``: the
    rollout is one captured graph and equals an eager twin, whose thief column is held against ``navigate_step`` on every tick."""
    run_step("opponent", 180)


def test_the_evaluation_pass_and_watch_play_navigators():
    """``evaluate_against_navigators`` on squarinth 2v1 x 16 slots: five match-ups without a source, all seven with a trainer's policies, every
    first episode counted once; ``watch(navigators={"cop": "pursue", "thief": "flee"})`` on two slots for 12 ticks."""
    run_step("users", 180)
