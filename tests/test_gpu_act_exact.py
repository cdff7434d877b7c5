"""GPU: the fused act tick (``cat_act_step``, ``cat_act_league_step``, ``cat_act_collect_step``; csrc/cat_act.hip) against an exactly
known answer.  tests/act_exact.py builds saturating networks and three-valued observations for which the layer-rounded fp64 reference
is what the kernel must produce bit for bit (magnitudes below 2^-24 count as 0); tests/test_act_exact_host.py holds the premises, the
coverage conditions and the teeth of that comparison on the CPU.  What is pinned here and nowhere else: the fragment-to-weight mappings
of the two convolutions, the (channel, position) flatten order, the gate row blocks, the [f | h] image, keep on h and c, the padded
logit tile, the per-network parameter stride, and round-to-nearest-even at every storage point.

Every step runs in a process of its own under its own time limit (tests/act_exact_steps.py); after a step that ended in a fault, an
abort or a time-out nothing more is started on the GPU: the remaining tests fail without running."""
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
        res = subprocess.run([sys.executable, "-m", "tests.act_exact_steps", step], cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as exc:
        FAULT["step"] = step
        pytest.fail(f"step {step!r} ran into its time limit of {seconds} s\n{exc.stdout}\n{exc.stderr}")
    print(res.stdout)
    print(res.stderr[-4000:], file=sys.stderr)
    if res.returncode not in (0, 1):                 # a signal, an abort, an interpreter error: not a failed check
        FAULT["step"] = step
    assert res.returncode == 0 and "ALL CHECKS PASSED" in res.stdout, f"step {step!r} exit {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-3000:]}"


def test_act_step_equals_the_exact_reference_over_eight_ticks():
    """R in {64, 90} x row tiles {32, 64} x N in {1, 33, 97}, three networks on agent columns [2, 0, 3] of four, greedy, keep and keep = NULL."""
    run_step("plain", 180)


def test_league_step_plays_every_row_with_its_own_set():
    """N = 97 in segments [0, 5, 38, 97], a bank of three sets, a different set per (policy, segment) and one random segment per policy."""
    run_step("league", 120)


def test_collect_step_equals_the_exact_reference_and_packs_the_scaled_rows():
    """R in {64, 90}, N = 33, first_agent_state both ways, a thief first in the agent order."""
    run_step("collect", 120)
