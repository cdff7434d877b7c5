"""CPU: the oracle's Space.step against the mechanical truth of tests/step_truth.py.

Every other env-core test compares the HIP kernels with oracle/cat_oracle.c, which restates Chipmunk's step and was written beside
the kernels: a misreading the two share (a contact threshold, a normal in a vertex region, an early-out, the bounding-box prune,
the bias formula, a sign in the pair impulse) would pass them all.  Here every tick of the scripted tapes of
tests/step_truth_cases.py is held against what follows from mechanics and geometry alone; tests/test_gpu_step_truth.py holds the
HIP library against the same truth without going through the oracle."""
import ast
from pathlib import Path

import numpy as np
import pytest

from tests import step_truth_cases as stc
from tests.step_truth import StepTruth, pair_indices

SQUARE = np.array([(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0)])


def test_the_truth_imports_only_numpy_and_the_ray_truth():
    tree = ast.parse((Path(__file__).resolve().parent / "step_truth.py").read_text())
    seen = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            seen |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "relative import"
            seen.add(node.module or "")
        elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in ("__import__", "import_module"):
            raise AssertionError("dynamic import")
    assert seen <= {"__future__", "numpy", "tests.ray_truth"}, seen


# ---- the truth's own primitives on cases a reader can check on paper ------------------------------------------------------------
def _truth():
    """reach = 2.5 + 1 = 3.5 px; an action changes a velocity by impulse / mass = 2; dt = 1/2"""
    return StepTruth([SQUARE], dt=0.5, mass=2.0, impulse=4.0, max_speed=100.0, agent_radius=2.5, wall_radius=1.0, bias_coef=0.25, slop=0.25)


def _state(pos, vel, vbias=None, walls=(), pairs=()):
    """One env; ``walls``: (agent, slot, shape, age, jn); ``pairs``: (pair index, age, jn).  Two cache slots per agent."""
    pos = np.array(pos, np.float64)[None]
    A = pos.shape[1]
    st = dict(pos=pos, vel=np.array(vel, np.float64)[None], vbias=np.zeros_like(pos) if vbias is None else np.array(vbias, np.float64)[None],
              wall_shape=np.full((1, A, 2), -1), wall_age=np.zeros((1, A, 2), int), wall_jn=np.zeros((1, A, 2)),
              pair_age=np.full((1, len(pair_indices(A))), -1), pair_jn=np.zeros((1, len(pair_indices(A)))))
    for a, k, s, age, jn in walls:
        st["wall_shape"][0, a, k], st["wall_age"][0, a, k], st["wall_jn"][0, a, k] = s, age, jn
    for q, age, jn in pairs:
        st["pair_age"][0, q], st["pair_jn"][0, q] = age, jn
    return st


def _zero(res, *keys):
    for k in keys:
        assert np.nanmax(res[k]) < 1e-14, (k, res[k])
    assert not res["missing"] and not res["extra"] and res["negative_jn"] == 0 and res["clear"].all()


def test_a_disc_pushed_square_into_a_face():
    """From (8, 2) at (-1, 0), pushed -x: v_in = (-3, 0), the centre lands at x = 6.5, 2.5 from the face x = 4: gap -1.  The contact
    takes all of the momentum 2 * 3 = 6, and pushes out with 0.25 * (1 - 0.25) / 0.5 = 0.375."""
    t = _truth()
    before = _state([(8.0, 2.0)], [(-1.0, 0.0)])
    after = _state([(6.5, 2.0)], [(0.0, 0.0)], [(0.375, 0.0)], walls=[(0, 0, 0, 0, 6.0)])
    res = t.tick(before, np.array([[0]]), after)
    _zero(res, "r_pos", "r_vel", "r_single_vel", "r_single_vbias")
    assert res["single"].all() and res["counts"]["vertex"] == 0 and res["counts"]["wall_contacts"] == 1
    # the same body without its cache entry, with an entry aged 1, bounced back, or pushed out as if the slop were 0
    assert t.tick(before, np.array([[0]]), _state([(6.5, 2.0)], [(0.0, 0.0)], [(0.375, 0.0)]))["missing"] == [(0, 0, 0)]
    assert t.tick(before, np.array([[0]]), _state([(6.5, 2.0)], [(0.0, 0.0)], [(0.375, 0.0)], walls=[(0, 0, 0, 1, 6.0)]))["missing"] == [(0, 0, 0)]
    res = t.tick(before, np.array([[0]]), _state([(6.5, 2.0)], [(3.0, 0.0)], [(0.5, 0.0)], walls=[(0, 0, 0, 0, 6.0)]))
    assert res["r_vel"][0, 0] == 3.0 and res["r_single_vel"][0, 0] == 3.0 and res["r_single_vbias"][0, 0] == 0.125
    # a body 4 px from the face has no contact: an entry for it is extra, its velocity is v_in, its bias velocity 0
    far = t.tick(_state([(9.5, 2.0)], [(-1.0, 0.0)]), np.array([[0]]), _state([(8.0, 2.0)], [(-3.0, 0.0)], walls=[(0, 0, 0, 0, 0.0)]))
    assert far["extra"] == [(0, 0, 0)] and far["r_vel"][0, 0] == 0.0
    res = t.tick(_state([(9.5, 2.0)], [(-1.0, 0.0)]), np.array([[0]]), _state([(8.0, 2.0)], [(-3.0, 0.0)]))
    _zero(res, "r_pos", "r_vel", "r_free_vbias")
    assert res["free"].all()


def test_a_disc_against_a_3_4_5_corner():
    """The centre lands at (5.8, 6.4), 3 from the corner (4, 4) along (0.6, 0.8): gap -0.5.  v_in = (-3, -4) = -5 n is all normal and
    is taken away (jn = 2 * 5 = 10); the push out is 0.25 * (0.5 - 0.25) / 0.5 = 0.125 along n."""
    t = _truth()
    before = _state([(7.3, 8.4)], [(-3.0, -2.0)])
    after = _state([(5.8, 6.4)], [(0.0, 0.0)], [(0.075, 0.1)], walls=[(0, 1, 0, 0, 10.0)])
    res = t.tick(before, np.array([[3]]), after)
    _zero(res, "r_pos", "r_vel", "r_single_vel", "r_single_vbias")
    assert res["counts"]["vertex"] == 1 and res["counts"]["slanted_edge"] == 0
    # with the face's normal (1, 0) in the vertex region the body would keep (0, -4) and lose jn = 6
    res = t.tick(before, np.array([[3]]), _state([(5.8, 6.4)], [(0.0, -4.0)], [(0.125, 0.0)], walls=[(0, 1, 0, 0, 6.0)]))
    assert res["r_vel"][0, 0] > 1.0 and res["r_single_vel"][0, 0] == pytest.approx(4.0) and res["r_single_vbias"][0, 0] == pytest.approx(0.1)
    # 3.5 from the corner is the threshold itself: not clear; a centre inside the hull neither
    on = _state([(4.0 + 2.1, 4.0 + 2.8)], [(0.0, 0.0)])
    assert not t.tick(on, np.array([[0]]), on)["clear"].any()
    inside = _state([(2.0, 1.0)], [(0.0, 0.0)])
    assert not t.tick(inside, np.array([[0]]), inside)["clear"].any()


def test_two_discs_head_on():
    """Equal masses at (3, 0) and (-1, 0), 4 apart after the move (they touch below 5): both leave at (1, 0), the impulse is 2 * 2 = 4,
    taken from body 0 and given to body 1 along the centre line."""
    t = _truth()
    before = _state([(18.5, 20.0), (24.5, 20.0)], [(1.0, 0.0), (1.0, 0.0)])
    after = _state([(20.0, 20.0), (24.0, 20.0)], [(1.0, 0.0), (1.0, 0.0)], pairs=[(0, 0, 4.0)])
    res = t.tick(before, np.array([[2, 0]]), after)
    _zero(res, "r_pos", "r_vel")
    assert res["counts"]["pair_contacts"] == 1 and not res["single"].any() and not res["free"].any()
    # the impulse with its sign flipped on body 1: body 1 would leave at (-3, 0)
    flipped = _state([(20.0, 20.0), (24.0, 20.0)], [(1.0, 0.0), (-3.0, 0.0)], pairs=[(0, 0, 4.0)])
    res = t.tick(before, np.array([[2, 0]]), flipped)
    assert res["r_vel"][0].tolist() == [0.0, 4.0]
    assert t.tick(before, np.array([[2, 0]]), _state([(20.0, 20.0), (24.0, 20.0)], [(3.0, 0.0), (-1.0, 0.0)]))["missing"] == [(0, ("pair", 0))]
    # found again at age 2 with 3 left in it: this tick's impulse is 7 - 3
    stale = _state([(18.5, 20.0), (24.5, 20.0)], [(1.0, 0.0), (1.0, 0.0)], pairs=[(0, 2, 3.0)])
    res = t.tick(stale, np.array([[2, 0]]), _state([(20.0, 20.0), (24.0, 20.0)], [(1.0, 0.0), (1.0, 0.0)], pairs=[(0, 0, 7.0)]))
    _zero(res, "r_vel")
    assert res["counts"]["pair_refound_nonzero"] == 1
    # a coincident pair has no centre line: both bodies not clear
    same = _state([(20.0, 20.0), (20.0, 20.0)], [(0.0, 0.0), (0.0, 0.0)])
    assert not t.tick(same, np.array([[2, 0]]), same)["clear"].any()


def test_a_glancing_contact_keeps_the_tangent():
    """v_in = (-3, 4) into the face x = 4: the normal part goes, the tangent (0, 4) stays; leaving at (1, 4) nothing changes; leaving a
    re-found wall whose stale entry holds 5 = 2 * 2.5, the body is held back by min(2.5, 1) and the entry is drawn down to 3."""
    t = _truth()
    res = t.tick(_state([(8.0, 0.0)], [(-1.0, 4.0)]), np.array([[0]]), _state([(6.5, 2.0)], [(0.0, 4.0)], [(0.375, 0.0)], walls=[(0, 0, 0, 0, 6.0)]))
    _zero(res, "r_pos", "r_vel", "r_single_vel", "r_single_vbias")
    res = t.tick(_state([(6.0, 0.0)], [(-1.0, 4.0)]), np.array([[2]]), _state([(6.5, 2.0)], [(1.0, 4.0)], [(0.375, 0.0)], walls=[(0, 0, 0, 0, 0.0)]))
    _zero(res, "r_pos", "r_vel", "r_single_vel", "r_single_vbias")
    stale = _state([(6.0, 0.0)], [(-1.0, 4.0)], walls=[(0, 0, 0, 2, 5.0)])
    res = t.tick(stale, np.array([[2]]), _state([(6.5, 2.0)], [(0.0, 4.0)], [(0.375, 0.0)], walls=[(0, 0, 0, 0, 3.0)]))
    _zero(res, "r_pos", "r_vel", "r_single_vel", "r_single_vbias")
    assert res["counts"]["single_refound_nonzero"] == 1
    # warm-started (age 0 before) the same entry gives the whole of jn_after back: the body keeps (1, 4) and the entry ends at 0
    warm = _state([(6.0, 0.0)], [(-1.0, 4.0)], walls=[(0, 0, 0, 0, 5.0)])
    res = t.tick(warm, np.array([[2]]), _state([(6.5, 2.0)], [(1.0, 4.0)], [(0.375, 0.0)], walls=[(0, 0, 0, 0, 0.0)]))
    _zero(res, "r_vel", "r_single_vel")
    # the speed clamp: (0, 99) pushed +y is (0, 101), clamped to 100
    res = t.tick(_state([(30.0, 0.0)], [(0.0, 99.0)]), np.array([[1]]), _state([(30.0, 50.0)], [(0.0, 100.0)]))
    _zero(res, "r_pos", "r_vel")


# ---- the oracle on every tape ------------------------------------------------------------------------------------------------------
TOTAL = {}


@pytest.mark.parametrize("name", stc.CASES)
def test_oracle_step_on_every_tape_with_its_coverage(name):
    """Counted by the truth's own geometry on clear bodies (150 ticks; the whole lines are in profiles/step_truth.txt):
    labyrinth_2v1_mixed / _units: single 1038, multi 112, vertex 51, pair and wall 8, 32 of 9000 agent-ticks not clear (the bodies where
                                  three walls overlap stand inside a hull); squarinth_1v1: single 542; grandbyrinth_3v2: single 581;
    random_12_2v1: single 980, vertex 35, slanted edge 375; lbirinth_2v1: single 541; agh-map_2v1: single 728, over two walls 14;
    bounce_labyrinth_2v1: single 554, wall re-finds 524 (523 on a single-contact body), pair re-finds 98, every one with a stale
                          impulse above 0.  Worst residuals over all tapes: pos 2.3e-13, vel 1.8e-12, single vel 3.1e-12, single vbias 3.5e-12."""
    s = stc.run_case(stc.oracle_sim, name)
    print(name, s["counts"])
    stc.check_least(name, s["counts"])
    TOTAL[name] = s["counts"]


def test_the_tapes_together_cover_what_the_truth_is_there_for():
    """(after the cases above; alone it replays them)"""
    for name in stc.CASES:
        if name not in TOTAL:
            TOTAL[name] = stc.run_case(stc.oracle_sim, name)["counts"]
    total = {k: sum(c[k] for n, c in TOTAL.items() if n != "labyrinth_2v1_units") for k in stc.LEAST_TOTAL}   # (the two labyrinth tapes are one tape)
    print("step-truth coverage over all tapes:", total)
    for k, n in stc.LEAST_TOTAL.items():
        assert total[k] >= n, (k, total)


def test_oracle_step_with_respawns_between_the_ticks():
    """The scenario of ``cat_step_fused(auto_reset=1)`` on the oracle's step + masked reset: slots whose episode ended in a tick are
    left out of that tick, and go on from their spawn points."""
    s = stc.run_case(stc.oracle_sim, "labyrinth_2v1_mixed", entry="fused", auto_reset=True, tag="step + respawn")
    assert not s["kept"].all() and s["kept"].mean() > 0.9, s["kept"].mean()


def test_oracle_holds_a_body_that_leaves_a_refound_wall_by_the_stale_impulse():
    stc.stale_leave_case(stc.oracle_sim)


# Measured on this test's own run (the oracle on the bounce tape, where every contact is a fraction of a pixel deep, and on the
# random-polygon tape): a truth whose agent radius is 4.9 for 5.0 finds the share RADIUS_MEASURED of the age-0 wall and pair entries
# outside its contact set (to it they are no contacts: they land in "extra"; with the right radius none does, and none is "missing");
# a truth with slop 0 for 0.1 disagrees on the share SLOP_MEASURED of the single-contact bias velocities (every contact is below
# its threshold, so every bias differs).  The floors are half of what was measured.
RADIUS_MEASURED = {"bounce_labyrinth_2v1": 0.582, "random_12_2v1": 0.058}   # 382 of 656; 73 of 1266
SLOP_MEASURED = {"bounce_labyrinth_2v1": 1.0, "random_12_2v1": 1.0}         # 554 of 554; 980 of 980


@pytest.mark.parametrize("name", list(RADIUS_MEASURED))
def test_a_tenth_of_a_pixel_in_the_agent_radius_and_the_slop_are_seen(name):
    """The check has teeth: the same comparison against a truth with a disc 0.1 px too small, or with no slop, must fail on a clear
    share of the contacts (and the right parameters on none)."""
    tr = stc.trace(name)
    states = stc.replay(stc.oracle_sim, tr)
    right, _ = stc.against_truth(stc.truth_for(tr.cmap, tr.cfg), states, tr.actions)
    assert not right["missing"] and not right["extra"]
    assert not (np.where(right["single"], right["r_single_vbias"], 0.0) > stc.TOL_VEL).any()
    small, _ = stc.against_truth(stc.truth_for(tr.cmap, tr.cfg, agent_radius=tr.cfg.agent_radius - 0.1), states, tr.actions)
    noslop, _ = stc.against_truth(stc.truth_for(tr.cmap, tr.cfg, slop=0.0), states, tr.actions)
    entries = right["counts"]["wall_contacts"] + right["counts"]["pair_contacts"]
    radius_share = (len(small["extra"]) + len(small["missing"])) / entries
    wrong_bias = int((np.where(noslop["single"], noslop["r_single_vbias"], 0.0) > stc.TOL_VEL).sum())
    slop_share = wrong_bias / int(noslop["single"].sum())
    line = (f"step-truth sensitivity {name}: agent radius 4.9 for 5.0 leaves {len(small['extra'])} extra + {len(small['missing'])} missing of {entries} "
            f"contacts outside the truth's set ({100 * radius_share:.1f} %); slop 0 for 0.1 changes {wrong_bias} of {int(noslop['single'].sum())} "
            f"single-contact bias velocities ({100 * slop_share:.1f} %)")
    stc.REPORT.append(line)
    print(line)
    assert radius_share >= RADIUS_MEASURED[name] / 2 > 0.02
    assert slop_share >= SLOP_MEASURED[name] / 2 > 0.02
