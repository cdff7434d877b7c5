"""The scripted Space.step scenarios (tests/space_step_cases.py) on the CPU: the oracle-side coverage counting runs without a GPU, and every
case's inputs contain what the GPU tests (tests/test_gpu_space_step_batch.py) are there to check."""
import numpy as np
import pytest

from tests import space_step_cases as cases


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_covers_the_solver_shapes_and_mixed_workgroups(name):
    """Counted from the oracle's states (slot ticks of 150 ticks):
    labyrinth_2v1_mixed / _units (20 envs): wall 931, two_on_one 109, two_agents 242, pair 87, over_bound 11, pair_and_wall 8, wall_expired 45, pair_expired 10,
                                            free beside a contact slot 1860 of 3000;
    squarinth_1v1 (16 envs):                wall 469, two_on_one 8, two_agents 97, pair 52, over_bound 0, pair_and_wall 10, wall_expired 21, pair_expired 3,
                                            free beside a contact slot 1889 of 2400;
    grandbyrinth_3v2 (16 envs):             wall 482, two_on_one 17, two_agents 122, pair 77, over_bound 0, pair_and_wall 13, wall_expired 22, pair_expired 10,
                                            free beside a contact slot 1850 of 2400.
    over_bound (a body with more wall contacts than the register solver takes): the labyrinth has a place where three wall shapes overlap, and two bodies
    are put there; on the two square maps at most two walls meet, so their cases ask for none."""
    tr = cases.trace(name)
    print(name, tr.coverage)
    cases.check_coverage(tr.coverage, tr.min_over_bound)
    assert tr.calm.any() and not tr.calm.all()
    assert (tr.placed != tr.start).any()                      # some bodies were moved onto walls before tick 0 ...
    first = tr.states[0]
    assert ((first["wall_shape"] >= 0) & (first["wall_age"] == 0)).any()   # ... so tick 0 already has contact slots beside free ones
    assert tr.actions.min() >= 0 and tr.actions.max() <= 3


def test_coverage_counts_a_hand_made_trace():
    """two envs, one body, K = 2 cache entries: a contact in env 0 at tick 0 that ages and expires; env 1 stays free"""
    def st(shape, age, page):
        return dict(wall_shape=np.array(shape).reshape(2, 1, 2), wall_age=np.array(age).reshape(2, 1, 2), pair_age=np.array(page).reshape(2, 1))
    states = [st([[4, 7], [-1, -1]], [[0, 0], [0, 0]], [-1, 0]),
              st([[4, 7], [-1, -1]], [[1, 0], [0, 0]], [-1, 1]),
              st([[-1, -1], [-1, -1]], [[0, 0], [0, 0]], [-1, -1])]
    c = cases.coverage(states)
    assert c["pair_and_wall"] == 0
    assert c["slot_ticks"] == 6 and c["wall"] == 2 and c["two_on_one"] == 1 and c["two_agents"] == 0
    assert c["pair"] == 1 and c["wall_expired"] == 2 and c["pair_expired"] == 1
    assert c["free_beside_contact"] == 1      # tick 1: env 1 free beside env 0; tick 0: both have a contact; tick 2: no contact slot
    assert c["over_bound"] == 0
