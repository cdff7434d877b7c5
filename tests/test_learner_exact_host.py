"""CPU: the premises of tests/test_gpu_learner_exact.py and the teeth of its comparisons.

1. Every exact case stays inside its exactness bounds (integers <= 256 where a kernel rounds an intermediate to bf16,
   partial sums below 2^22), worked out from the generators' value ranges: a later change of shapes or ranges cannot
   silently turn an exact test into a flaky one.
2. Synthetic defects, applied to fp64 reference results on the CPU, are rejected by the exact comparison although the
   tolerances the older tests use accept them: a truncating bf16 conversion, a ">= 0" ReLU mask, one dropped sample at
   a ragged tail, one dropped k-row; and the LSTM per-row bound rejects one (t, b) with the wrong keep handling."""
import pytest

torch = pytest.importorskip("torch")

from tests import learner_exact as lx  # noqa: E402


# ---------------------------------------------------------------------------------------------- 1. premises
@pytest.mark.parametrize("c", lx.dense_cases(), ids=lambda c: c.id)
def test_dense_cases_are_exact(c):
    for name, (got, limit) in lx.dense_bounds(c).items():
        assert got <= limit, (name, got, limit)


@pytest.mark.parametrize("K", sorted({k for _, k, _, _ in lx.WGRAD_CASES} | {k for _, k, _, _, _ in lx.WGRAD2_CASES}))
def test_weight_gradient_cases_are_exact(K):
    for name, (got, limit) in lx.wgrad_bounds(K).items():
        assert got <= limit, (name, got, limit)


@pytest.mark.parametrize("c", lx.trunk_cases(), ids=lambda c: c.id)
def test_trunk_cases_are_exact(c):
    w1, b1, w2, _ = lx.trunk_params(c, c.N + 10 * c.C + c.R)
    for name, (got, limit) in lx.trunk_bounds(c, w1, b1, w2).items():
        assert got <= limit, (name, got, limit)
    assert lx.trunk_nnz(c, lx.trunk_z1_max(w1, b1)) >= 1


def test_the_premises_hold_on_drawn_data_too():
    """Small versions of the generators, worked through in fp64: the intermediates the kernels round to bf16 are
    integers inside the bounds, and the ReLU layers meet pre-activations of exactly 0 often."""
    c = lx.DenseCase(2, 4096, 256, 128, lx.ACT_RELU, True)
    d = lx.dense_data(c, 1, "cpu")
    ref = lx.dense_reference(c, d)
    pre = ref["prod"] + d["b"].unsqueeze(1)
    assert float((pre == 0).double().mean()) > 0.02
    assert torch.equal(lx.rne_bf16(ref["g"]).double(), ref["g"])
    t = lx.TrunkCase(1, 300, 4, 90)
    w1, b1, w2, b2 = lx.trunk_params(t, 9)
    x, dout = lx.trunk_inputs(t, 9, "cpu", lx.trunk_z1_max(w1, b1))
    z1 = torch.relu(torch.einsum("nclk,ock->nol", x[0].view(-1, 4, 90).unfold(2, 5, 2), w1[0]) + b1[0].view(1, -1, 1))
    assert float(z1.max()) <= lx.trunk_z1_max(w1, b1) <= lx.BF16_INT and float((z1 == 0).double().mean()) > 0.05
    assert int((dout != 0).sum(2).max()) <= lx.trunk_nnz(t, lx.trunk_z1_max(w1, b1))


@pytest.mark.parametrize("gamma,lam,T", lx.GAE_CASES)
def test_gae_cases_are_exact_in_fp32(gamma, lam, T):
    assert lx.gae_bits(T, gamma, lam, lx.GAE_VMAX) <= 24
    gen = torch.Generator().manual_seed(T)
    v = lx.GAE_VMAX
    rew = torch.randint(-v, v + 1, (2, T, 64), generator=gen).double()
    val = torch.randint(-v, v + 1, (2, T, 64), generator=gen).double()
    last = torch.randint(-v, v + 1, (2, 64), generator=gen).double()
    dones = torch.rand(T, 64, generator=gen) < 0.2
    adv, ret = lx.gae_reference(rew, val, dones, last, gamma, lam)
    assert torch.equal(adv.float().double(), adv) and torch.equal(ret.float().double(), ret)


def test_sampler_uniforms_meet_the_cdf_exactly():
    """With masses exactly 1 (sum 4) the products u * sum of the chosen uniforms are exact in fp32 and land on the cdf
    values themselves at 1/4, 1/2, 3/4: the tie convention is what decides those draws."""
    for u in lx.UNIFORMS:
        assert float(torch.tensor(u, dtype=torch.float32) * 4) == u * 4
    assert {u * 4 for u in lx.UNIFORMS} >= {1.0, 2.0, 3.0}
    # with an underflowed trailing mass the sum equals the last cdf value: u = 1 - 2^-24 times any sum of up to four
    # masses stays below that sum in fp32 (round to nearest even), so the zero-mass action is never reached
    for s in (1.0, 2.0, 3.0, 4.0, 1.5, 2.75, 3.0000002):
        t = torch.tensor(s, dtype=torch.float32)
        assert float(torch.tensor(lx.UNIFORMS[-1], dtype=torch.float32) * t) < float(t)


# ---------------------------------------------------------------------------------------------- 2. teeth
def _random_wgrad(K, M, N, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(1, K, M, generator=gen).to(torch.bfloat16).double()
    x = (torch.randn(1, K, N, generator=gen) + 0.5).to(torch.bfloat16).double()
    return g, x


def test_a_truncating_bf16_conversion_is_rejected():
    """Weight gradient of the (3, 4096, 256, 288) shape of test_gpu_dense_kernels.py: truncated instead of rounded."""
    K, M, N = 4096, 256, 288
    g, x = _random_wgrad(K, M, N, 0)                    # the older test's data: its tolerance accepts the defect ...
    want = torch.bmm(g.transpose(1, 2), x)
    assert lx.old_gemm_tolerance(lx.trunc_bf16(want), want)
    gen = torch.Generator().manual_seed(1)              # ... the exact data does not
    g = torch.randint(-2, 3, (1, K, M), generator=gen).double()
    x = torch.randint(-2, 3, (1, K, N), generator=gen).double()
    want = torch.bmm(g.transpose(1, 2), x)
    assert lx.exact_equal(lx.rne_bf16(want), want) and not lx.exact_equal(lx.trunc_bf16(want), want)


def test_a_greater_or_equal_relu_mask_is_rejected():
    """The ReLU derivative taken as 1 at a pre-activation of exactly 0 (">= 0") instead of torch's 0 (threshold_backward:
    gradient only where the output is > 0): continuous data never has a pre-activation of exactly 0, so the older tests
    cannot see it; the exact data has many."""
    def grads(d, ge):
        pre = torch.bmm(d["x"], d["w"].transpose(1, 2)) + d["b"].unsqueeze(1)
        g = d["d_y"] * ((pre >= 0) if ge else (torch.relu(pre) > 0)).double()
        return g, g.sum(1), torch.bmm(g.transpose(1, 2), d["x"])
    c = lx.DenseCase(1, 2048, 128, 64, lx.ACT_RELU, True)
    gen = torch.Generator().manual_seed(2)
    rnd = {"x": torch.randn(1, 2048, 128, generator=gen).to(torch.bfloat16).double(),
           "w": torch.randn(1, 64, 128, generator=gen).to(torch.bfloat16).double(),
           "b": torch.randn(1, 64, generator=gen).to(torch.bfloat16).double(),
           "d_y": torch.randn(1, 2048, 64, generator=gen).to(torch.bfloat16).double()}
    assert all(torch.equal(a, b) for a, b in zip(grads(rnd, False), grads(rnd, True)))
    d = lx.dense_data(c, 3, "cpu")
    ref = lx.dense_reference(c, d)
    g_bad, db_bad, dw_bad = grads(d, True)
    assert not lx.exact_equal(lx.rne_bf16(g_bad), ref["g"])
    assert not lx.exact_equal(lx.rne_bf16(db_bad), ref["db"]) and not lx.exact_equal(lx.rne_bf16(dw_bad), ref["dw"])


def _old_trunk_case(N, C, R, seed):
    """test_gpu_trunk_kernels._case on the CPU: the older test's data and scales."""
    gen = torch.Generator().manual_seed(seed)
    bfr = lambda t: t.to(torch.bfloat16).double()
    x = bfr(torch.rand(1, N, C * R, generator=gen))
    w1, b1 = bfr(0.4 * torch.randn(1, 64, C, 5, generator=gen)), bfr(0.2 * torch.randn(1, 64, generator=gen))
    w2, b2 = bfr(0.08 * torch.randn(1, 32, 64, 5, generator=gen)), bfr(0.2 * torch.randn(1, 32, generator=gen))
    return x, (w1, b1, w2, b2)


def test_one_dropped_sample_at_a_ragged_tail_is_rejected():
    """The last sample of N = 4099 (a partial 16-sample tile) left out of every parameter gradient."""
    N, C, R = 4099, 4, 64
    c = lx.TrunkCase(1, N, C, R)
    x, p = _old_trunk_case(N, C, R, 4)
    d = torch.randn(1, N, c.L2 * 32, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).double()
    _, want = lx.trunk_reference(c, x, *p, d)
    _, bad = lx.trunk_reference(c, x, *p, torch.cat([d[:, :-1], torch.zeros_like(d[:, -1:])], 1))
    assert lx.old_grad_tolerance(bad[0], want[0]) and lx.old_grad_tolerance(bad[1], want[1])     # d_w1, d_b1 pass the old bar
    w1, b1, w2, b2 = lx.trunk_params(c, 6)
    x, d = lx.trunk_inputs(c, 6, "cpu", lx.trunk_z1_max(w1, b1))
    d[:, -1] = 0
    d[:, -1, :32] = 1                                    # the tail sample reaches every first-layer channel
    _, want = lx.trunk_reference(c, x, w1, b1, w2, b2, d)
    _, bad = lx.trunk_reference(c, x, w1, b1, w2, b2, torch.cat([d[:, :-1], torch.zeros_like(d[:, -1:])], 1))
    assert all(lx.exact_equal(lx.rne_bf16(w), w) for w in want)
    assert not lx.exact_equal(lx.rne_bf16(bad[2]), want[2]) and not lx.exact_equal(lx.rne_bf16(bad[3]), want[3])


def test_one_dropped_k_row_is_rejected():
    """One row of a 16384-row weight-gradient reduction left out (row 5000 of the exact data; for the older test's data a
    row whose products are small, as most of them are next to the 2^-7 x max |want| tolerance)."""
    K, M, N = 16384, 128, 64
    g, x = _random_wgrad(K, M, N, 7)
    want = torch.bmm(g.transpose(1, 2), x)
    k = int((g[0].abs().amax(1) * x[0].abs().amax(1)).argmin())      # a row whose products are small, not an empty one
    bad = want - g[:, k].unsqueeze(2) * x[:, k].unsqueeze(1)
    assert float(bad.sub(want).abs().max()) > 0 and lx.old_gemm_tolerance(lx.rne_bf16(bad), want)
    gen = torch.Generator().manual_seed(8)
    g = torch.randint(-2, 3, (1, K, M), generator=gen).double()
    x = torch.randint(-2, 3, (1, K, N), generator=gen).double()
    want = torch.bmm(g.transpose(1, 2), x)
    bad = want - g[:, 5000].unsqueeze(2) * x[:, 5000].unsqueeze(1)
    assert not lx.exact_equal(lx.rne_bf16(bad), want)


def test_the_lstm_row_bound_rejects_one_wrong_keep():
    """fp64 recurrence with keep ignored at one (t, b) against the right one: the per-row bound with the calibrated k
    rejects it (out and the gradients), while the right recurrence rounded to bf16 passes."""
    from tests.test_gpu_lstm_kernels import LSTM_K
    G, T, B, H = 1, 16, 32, 128
    gen = torch.Generator().manual_seed(11)
    xproj = torch.randn(G, T, B, 4 * H, generator=gen).to(torch.bfloat16).double()
    w_hh = (0.15 * torch.randn(G, 4 * H, H, generator=gen)).to(torch.bfloat16).double()
    h0 = (0.5 * torch.randn(G, B, H, generator=gen)).to(torch.bfloat16).double()
    c0 = torch.randn(G, B, H, generator=gen).to(torch.bfloat16).double()
    keep = (torch.rand(T, B, generator=gen) > 0.2).double()
    keep[5, 7] = 0.0
    bad_keep = keep.clone()
    bad_keep[5, 7] = 1.0
    r = torch.randn(G, T, B, H, generator=gen, dtype=torch.float64)

    def run(k):
        leaves = [t.clone().requires_grad_(True) for t in (xproj, h0, c0)]
        out, _, _ = lx.lstm_reference(leaves[0], w_hh, leaves[1], leaves[2], k)
        (out * r).sum().backward()
        return out.detach(), leaves[0].grad
    out, dx = run(keep)
    bad_out, bad_dx = run(bad_keep)
    assert lx.row_k(out.to(torch.bfloat16), out) <= 1.0 and lx.row_k(dx.to(torch.bfloat16), dx) <= 1.0
    assert lx.row_k(bad_out, out) > LSTM_K["out"]
    assert lx.row_k(bad_dx, dx) > LSTM_K["d_xproj"]
