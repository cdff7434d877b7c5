"""CPU: the premises of tests/test_gpu_act_exact.py, its coverage conditions and the teeth of its comparison (tests/act_exact.py).

1. Every case's data meets the premises that make the kernel's right answer exactly known, and the coverage conditions that make
   the data able to see a defect.  One condition is replaced in the one-row cases, and only that one: "keep = 0 on at least 15 %
   of the rows of every tick after the first" would there reset the state in every tick and leave W_hh nothing to act on, so they
   are asked instead that keep = 0 meets a nonzero state in at least one tick after the first and keep = 1 does in at least one.
2. The layer-rounded reference agrees with ``reference_tick`` of tests/act_steps.py (no rounding, no flush), the formulation the
   accuracy step already uses, to 2^-7 of the largest logit.
3. Ten defects in the index arithmetic, applied to the reference, are all rejected by ``act_equal`` on the logits or the state."""
import pytest

torch = pytest.importorskip("torch")

from tests import act_exact as ax  # noqa: E402
from tests import learner_exact as lx  # noqa: E402

CASES = ax.data_cases()
_CACHE = {}


def case_data(c):
    if c.seed not in _CACHE:
        P, d = ax.make_params(c.sets, c.R, c.seed), ax.make_inputs(c)
        _CACHE[c.seed] = (P, d, ax.reference(c, P, d, details=True))
    return _CACHE[c.seed]


def test_the_cases_are_the_ones_the_gpu_steps_run():
    ids = {c.id for c in ax.all_cases()}
    assert len(ids) == len(ax.all_cases()) == 12 + 4 + 4
    assert {(c.R, c.row_tile, c.N) for c in ax.plain_cases()} == {(R, t, N) for R in (64, 90) for t in (32, 64) for N in (1, 33, 97)}
    assert all(c.G == 3 and c.A == 4 and c.agents == (2, 0, 3) and c.T == 8 for c in ax.all_cases())
    assert all(c.N == 97 for c in ax.league_cases()) and ax.SEG_START == (0, 5, 38, 97)
    assert all(b % 32 for b in ax.SEG_START[1:-1]) and all(sorted(row)[0] == -1 and len(set(row)) == 3 for row in ax.SEG_SET)
    assert all(len({ax.SEG_SET[g][s] for g in range(3)}) == 3 for s in range(3))
    assert {(c.R, c.N, c.first_agent_state) for c in ax.collect_cases()} == {(R, 33, f) for R in (64, 90) for f in (False, True)}
    assert ax.AGENTS[0] >= ax.N_COPS                              # a thief first in the agent order
    assert ax.DISTANCE_SCALE != ax.TYPE_SCALE


def test_the_parameter_names_are_the_bindings():
    from as_cops_and_thieves_amd import _learn_native as ln
    assert ax.NAMES == ln.ACT_PARAM_NAMES and ax.HID == ln.HIDDEN


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_premises_and_coverage(c):
    P, d, ref = case_data(c)
    prem, cov, fig = ax.premises(c, P, d, ref), ax.coverage(c, P, d, ref), ax.figures(c, P, d, ref)
    for name, (value, limit) in prem.items():
        print(f"{c.id}: premise  {name}: {value:.6g} (limit {limit:.6g})")
    for name, (value, lo, hi) in cov.items():
        print(f"{c.id}: coverage {name}: {value:.6g} (allowed {lo:.6g} .. {hi:.6g})")
    for name, value in fig.items():
        print(f"{c.id}: figure   {name}: {value:.6g}")
    for name, (value, limit) in prem.items():
        assert ax.premise_holds(name, value, limit), (name, value, limit)
    for name, (value, lo, hi) in cov.items():
        assert lo <= value <= hi, (name, value, lo, hi)    # the observations become {0, 1, 2} on both channels, through different scales
    x = ax.policy_rows(c, d, 0)
    assert set(x[..., :c.R].unique().tolist()) == set(x[..., c.R:].unique().tolist()) == {0.0, 1.0, 2.0}
    assert set(d["obs_distance"].unique().tolist()) != set(d["obs_type"].unique().tolist())


@pytest.mark.parametrize("R", (64, 90))
def test_the_parameter_buffer_is_what_act_params_takes(R):
    P = ax.make_params(3, R, 7)
    flat = ax.flat_params(P, R)
    views = ax.param_views(flat, R)
    off, stride = ax.param_layout(R)
    assert stride % 8 == 0 and ax.BAND % 8 == 0 and all(o % 8 == 0 for o in off.values())
    assert bool(flat[:ax.BAND].isnan().all()) and bool(flat[-ax.BAND:].isnan().all())
    for n in ax.NAMES:
        v = views[n]
        assert v.dtype == torch.bfloat16 and v[0].is_contiguous() and v.stride(0) == stride and v.data_ptr() % 16 == 0
        assert torch.equal(v.double(), P[n])
    assert not torch.equal(P[ax.NAMES[4]][0], P[ax.NAMES[4]][1])          # per-network distinct


@pytest.mark.parametrize("c", [c for c in CASES if c.form != "league"], ids=lambda c: c.id)
def test_the_reference_agrees_with_reference_tick(c):
    """Its own state carried through the T ticks.  (reference_tick plays network g on all rows of policy g: the plain and collect data.)"""
    from tests.act_steps import reference_tick
    P, d, ref = case_data(c)
    h, cc = d["h0"].clone(), d["c0"].clone()
    for t in range(c.T):
        z, h, cc = reference_tick(P, ax.policy_rows(c, d, t), h, cc, d["keep"][t].double(), c.R)
        err, scale = float((ref[t]["logits"] - z).abs().max()), float(z.abs().max())
        assert err <= 2.0 ** -7 * scale, (t, err, scale)


@pytest.mark.parametrize("mut", ax.MUTANTS)
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_a_defect_in_the_index_arithmetic_is_rejected(c, mut):
    P, d, ref = case_data(c)
    bad = ax.reference(c, P, d, mut=mut)
    assert all(ax.act_equal(ref[t][k], ref[t][k]) for t in range(c.T) for k in ("logits", "h", "c"))
    assert not all(ax.act_equal(bad[t][k], ref[t][k]) for t in range(c.T) for k in ("logits", "h", "c"))


def test_act_equal_is_bit_exact_away_from_zero_and_bounded_at_zero():
    want = torch.tensor([1.0, 0.76171875, 0.0, 0.0, -3.0], dtype=torch.float64)
    ok = want.clone()
    ok[2], ok[3] = 2.0 ** -24, -1e-12
    assert ax.act_equal(ok.to(torch.bfloat16), want)
    for i, v in ((0, 1.0 + 2.0 ** -7), (1, 0.7578125), (2, 2.0 ** -23), (4, 3.0)):
        bad = ok.clone()
        bad[i] = v
        assert not ax.act_equal(bad.to(torch.bfloat16), want)
    assert ax.act_equal(lx.rne_bf16(torch.tensor([0.998046875 + 1e-9], dtype=torch.float64)), torch.tensor([1.0], dtype=torch.float64))
    assert float(ax.rounded(torch.tensor([3e-8, -3e-8, 6e-8], dtype=torch.float64)).abs().sum()) == float(torch.tensor(6e-8).to(torch.bfloat16))
    z = torch.tensor([[1.0, 2.0, 2.0, 0.0], [3.0, 3.0, 3.0, 3.0], [0.0, -1.0, 0.5, 0.5]], dtype=torch.float64)
    assert ax.first_max(z).tolist() == [1, 0, 2]
    assert ax.random_action(torch.tensor([0.0, 0.25, 0.9999999, 0.74])).tolist() == [0, 1, 3, 2]
