"""CPU: what the per-block gradient check of ``test_gpu_stacked_blocks.py`` rests on (``tests/stacked_blocks.py``).

  * the cap: for every case of the GPU test's list and every agent, 3 * nu <= 0.5 -- a condition the CASES must meet (change a
    case's shape or seed in the shared list if it does not; never the cap);
  * the power of the check: with the yardstick gradient standing in for a correct bf16 implementation, the per-block criterion
    rejects every block that is zeroed, doubled, swapped with the next agent's or with another block of its size, while the
    whole-vector criterion of ``test_gpu_mappo.py`` accepts at least half of the zeroed / doubled ones;
  * the helpers' name -> offset -> module mapping, on the CPU fp32 StackedNet that ``test_mappo_cpu.py`` already proves right.
"""
import warnings

import pytest
import torch

from tests import stacked_blocks as sb

warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")


def _losses(spec):
    return (False,) if spec.arch == "mlp" else (False, True)     # the non-recurrent pair has no final state


@pytest.mark.parametrize("spec", sb.CASES, ids=lambda s: s.id)
def test_three_times_the_yardstick_noise_stays_below_the_cap(spec):
    for with_state in _losses(spec):
        for g in range(spec.G):
            errs = sb.yardstick_errors(spec, g, with_state)
            nu = max(errs.values())
            print(f"{spec.id} agent {g} state-loss {with_state}: nu = {nu:.4f} ({max(errs, key=errs.get)})")
            assert nu > 0.0 and sb.FACTOR * nu <= sb.CAP, (spec.id, g, with_state, errs)


def _mutations(spec, grads, other):
    """(label, mutated {block: gradient}) for every block of one agent's yardstick gradient ``grads``; ``other`` = the next
    agent's.  The two bias vectors of one LSTM layer have EQUAL gradients by construction (the GPU test asserts identical
    bits), so "another block of the same size" is a block of another layer: the value network has one, the policy network none."""
    for n in grads:
        yield f"zero {n}", {**grads, n: torch.zeros_like(grads[n])}
        yield f"double {n}", {**grads, n: 2 * grads[n]}
        if other is not None:
            yield f"next agent's {n}", {**grads, n: other[n]}
        if n.startswith("lstm.bias_ih_l"):
            for m in grads:
                if m != n and m.startswith("lstm.bias_") and m[-1] != n[-1] and grads[m].numel() == grads[n].numel():
                    yield f"swap {n} with {m}", {**grads, n: grads[m], m: grads[n]}


@pytest.mark.parametrize("spec", sb.CASES, ids=lambda s: s.id)
def test_the_block_criterion_rejects_every_mutated_block_and_the_whole_vector_criterion_does_not(spec):
    case = sb.case_of(spec, "cpu", torch.float32)
    fp = case.fp
    n_mut = n_blind = n_zero_double = 0
    for with_state in _losses(spec):
        for g in range(spec.G):
            ref, yard = sb.reference_of(spec, g, with_state)[0], sb.yardstick_of(spec, g, with_state)[0]
            other = sb.yardstick_of(spec, (g + 1) % spec.G, with_state)[0] if spec.G > 1 else None
            bound = sb.FACTOR * sb.noise(spec, g, with_state)
            ref_row = sb.flat_of(fp, spec.kind, ref)
            fp.grad[g].copy_(sb.flat_of(fp, spec.kind, yard))
            assert max(sb.block_errors(fp, spec.kind, g, ref).values()) <= bound          # the unmutated gradient passes
            assert sb.whole_vector_check(fp.grad[g], ref_row)
            for label, mutated in _mutations(spec, yard, other):
                fp.grad[g].copy_(sb.flat_of(fp, spec.kind, mutated))
                errs = sb.block_errors(fp, spec.kind, g, ref)
                assert max(errs.values()) > bound, (spec.id, g, with_state, label, max(errs.values()), bound)
                n_mut += 1
                if label.startswith(("zero", "double")):
                    n_zero_double += 1
                    n_blind += sb.whole_vector_check(fp.grad[g], ref_row)
    print(f"{spec.id}: {n_mut} mutations rejected per block; the whole-vector criterion accepts {n_blind} of {n_zero_double} zeroed / doubled blocks")
    assert 2 * n_blind >= n_zero_double, (n_blind, n_zero_double)


@pytest.mark.parametrize("spec", sb.CASES, ids=lambda s: s.id)
def test_cpu_fp32_stacked_net_matches_fp64_per_block_through_the_same_helpers(spec):
    """Every block within 1e-4 relative of fp64 (the tolerance of ``test_stacked_networks_equal_the_per_agent_modules``), forward
    within 1e-5 of the output scale: the helpers read the right block for the right module parameter."""
    case = sb.case_of(spec, "cpu", torch.float32)
    for with_state in _losses(spec):
        out = sb.run_stacked(case, with_state)
        for g in range(spec.G):
            ref, out64 = sb.reference_of(spec, g, with_state)
            assert sorted(ref) == sorted(case.blocks)
            errs = sb.block_errors(case.fp, spec.kind, g, ref)
            assert max(errs.values()) <= 1e-4, (spec.id, g, with_state, errs)
            assert float((out[g].double() - out64).abs().max()) <= 1e-5 * float(out64.abs().max())
    assert not bool(case.fp.grad[:, sb.padding_columns(case.fp)].any())
