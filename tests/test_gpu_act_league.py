"""GPU: ``cat_act_league_step`` (include/cat_act.h), the fused ``LeagueActor``, ``evaluate_league`` and the cross-play table.  Every step
runs in a process of its own under its own time limit (``tests/league_steps.py``); after a step that ended in a fault, an abort or a
time-out nothing more is started on the GPU: the remaining tests fail without running."""
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
        res = subprocess.run([sys.executable, "-m", "tests.league_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_segments_equal_the_plain_entry_bit_for_bit():
    """Rosters (2, 1) at 64 rays and (3, 2) at 90, N = 150 in segments of 1, 15, 16, 17, 31, 33, 37 rows, a bank of 4 sets, both row
    tiles and both modes, guarded buffers: every (policy, segment) equals the plain entry's launch over all rows with that set; random
    entries leave their state and optional outputs alone; one segment with set g for policy g is the plain entry."""
    run_step("segments", 180)


def test_league_act_and_env_tick_replay_from_a_graph_bit_for_bit():
    run_step("graph", 120)


def test_league_pass_equals_each_cell_played_alone_and_crossplay_reproduces_it():
    run_step("end_to_end", 180)
