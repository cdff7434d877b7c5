"""GPU: ``cat_rollout_scripted`` (include/cat_rollout.h) against its torch form ``selfplay.scripted.scripted_step``, the fused
``ScriptedActor`` on an env, scripted agents in a fused ``LeagueActor``, and what the scripts are for.  Every step runs in a process of its
own under its own time limit (``tests/scripted_steps.py``); after a step that ended in a fault, an abort or a time-out nothing more is
started on the GPU: the remaining tests fail without running."""
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
        res = subprocess.run([sys.executable, "-m", "tests.scripted_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_kernel_gives_the_hand_derived_answers():
    """The cases of tests/scripted_cases.py (R = 8, answers derived from the rule's text) through the kernel, one row each."""
    run_step("hand", 60)


def test_kernel_equals_the_torch_form_on_random_buffers():
    """(N, A, G, R) = (1, 2, 2, 8), (67, 3, 3, 64), (33, 5, 5, 90), (5, 3, 2, 300); G = 2 with a non-identity agent map; three consecutive
    ticks with keep absent, half zero and mostly one; about a third of the rows see their target and some have every cone blocked:
    actions and state bit-equal after every tick."""
    run_step("random", 60)


def test_kernel_leaves_everything_else_untouched():
    """Columns of uncovered agents, rows of -1 segments, the inputs and the guard bands around every buffer keep what they held."""
    run_step("untouched", 60)


def test_a_segment_table_equals_one_launch_per_segment():
    run_step("segments", 60)


def test_a_captured_launch_replays_bit_for_bit():
    run_step("graph", 60)


def test_fused_actor_equals_the_torch_form_on_an_env_for_200_ticks():
    """Squarinth 2v1, 64 envs, 64 rays, 200 ticks with episode ends: action for action and state for state, every tick."""
    run_step("env", 90)


def test_scripted_segments_leave_the_network_segments_of_a_league_bit_equal():
    """A fused ``LeagueActor`` with mixed segments against the same match-ups with the scripted agents "random": the network-played cells
    (actions of three ticks, h, c, logits) are bit-equal, the scripted cells are the rule, the random cells stay min(3, int(4u))."""
    run_step("league", 90)


def test_chase_beats_random_and_evade_escapes_random():
    """The purpose.  Squarinth 2v1, 64 rays, 256 slots per match-up, first episode each, max_step_count 400, fixed seeds: chase cops win
    strictly more episodes against random thieves than random cops do, and random cops win strictly more against random thieves than
    against evade thieves (profiles/scripted.txt has the measured rates)."""
    run_step("purpose", 120)


def test_watch_plays_scripted_roles():
    """``watch(scripts={"cop": "chase", "thief": "evade"})`` on two slots for 12 ticks, through the trainer and through the fused actor."""
    run_step("watch", 120)
