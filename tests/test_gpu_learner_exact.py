"""GPU: exact known-answer tests of the learner kernels (csrc/cat_{dense,trunk,ppo,rollout}.hip).  Integer operands make
every product and partial sum exact (tests/learner_exact.py states and checks the premises), so each bf16 result must
equal the fp64 result rounded once to nearest even, BIT FOR BIT: a dropped or doubled k-row, split or sample, a wrong
tile or fragment mapping, a truncating conversion or a different ReLU convention at exactly zero all fail torch.equal.
The tolerance tests of the same kernels (test_gpu_{dense,trunk}_kernels.py) keep the random-data and tanh coverage."""
import pytest

torch = pytest.importorskip("torch")

from tests import learner_exact as lx  # noqa: E402

pytestmark = pytest.mark.gpu
bf = torch.bfloat16


def _premises(bounds):
    for name, (got, limit) in bounds.items():
        assert got <= limit, (name, got, limit)


def _strided(shape, fill, pad=8):
    """a [G, ...] view whose [...] blocks are contiguous rows of a wider flat buffer (as FlatParams slots), holding ``fill``;
    returns (view, flat) so the padding can be checked afterwards."""
    G, n = shape[0], int(torch.tensor(shape[1:]).prod())
    flat = torch.full((G, n + 2 * pad), 7.0, dtype=bf, device="cuda")
    v = flat[:, pad:pad + n].view(*shape)
    v.copy_(fill.to(bf))
    return v, flat


def _pad_intact(flat, pad=8):
    return bool((flat[:, :pad] == 7).all()) and bool((flat[:, -pad:] == 7).all())


# ---------------------------------------------------------------------------------------------- dense layers
@pytest.mark.parametrize("c", lx.dense_cases(), ids=lambda c: c.id)
def test_dense_layer_kernels_are_bit_exact_on_integer_data(c):
    """cat_dense_forward (with and without bias), cat_dense_bias_act, cat_dense_act_grad + cat_dense_sum_chunks (new and
    accumulated into a row-strided slot), cat_dense_dgrad, cat_dense_wgrad alone and with the fused bias job
    (cat_dense_sum_chunks2) against fp64 -> bf16 (RNE).  The layers of every net shape at the trainer's 131 072-row
    minibatch (the trunk's tanh flatten layer run with ReLU here) and the ragged shapes of test_gpu_dense_kernels.py."""
    from as_cops_and_thieves_amd import _learn_native as ln
    _premises(lx.dense_bounds(c))
    d = lx.dense_data(c, seed=c.M + 7 * c.K + c.N, device="cuda")
    ref = lx.dense_reference(c, d)
    if c.act == lx.ACT_RELU:       # the case exercises the convention at a pre-activation of exactly zero
        zeros = float((ref["prod"] + d["b"].unsqueeze(1) == 0).double().mean())
        assert zeros > 0.005, zeros
    x = d["x"].to(bf)
    w, wflat = _strided((c.G, c.N, c.K), d["w"])
    b = d["b"].to(bf)

    y = ln.dense_forward(x, w, b, c.act)
    assert lx.exact_equal(y, ref["y"]), "forward"
    if c.act == lx.ACT_NONE:
        assert lx.exact_equal(ln.dense_forward(x, w, None, 0), ref["prod"]), "forward without bias"
    p16 = lx.rne_bf16(ref["prod"])
    post = p16.double() + d["b"].unsqueeze(1)
    assert lx.exact_equal(ln.dense_bias_act_(p16.clone(), b, c.act), torch.relu(post) if c.act else post), "bias_act"

    g, part = ln.dense_act_grad(d["d_y"].to(bf), y, c.act)
    assert lx.exact_equal(g, ref["g"]), "act_grad"
    assert lx.exact_equal(ln.sum_chunks(part), ref["db"]), "sum_chunks"
    sb, sbflat = _strided((c.G, c.N), d["slot_b"])
    ln.sum_chunks(part, sb, accumulate=True)
    assert lx.exact_equal(sb, d["slot_b"] + ref["db"]) and _pad_intact(sbflat), "sum_chunks into a slot"

    assert lx.exact_equal(ln.dense_dgrad(g, w), ref["dx"]), "dgrad"
    assert lx.exact_equal(ln.dense_wgrad(g, x), ref["dw"]), "wgrad"
    sw, swflat = _strided((c.G, c.N, c.K), d["slot_w"])
    sb, sbflat = _strided((c.G, c.N), d["slot_b"])
    ln.dense_wgrad(g, x, sw, bias_job=(part, sb) if ln.wgrad_supported(g, x) else None)
    torch.cuda.synchronize()
    assert lx.exact_equal(sw, d["slot_w"] + ref["dw"]) and _pad_intact(swflat), "wgrad into a slot"
    if ln.wgrad_supported(g, x):
        assert lx.exact_equal(sb, d["slot_b"] + ref["db"]) and _pad_intact(sbflat), "bias job of wgrad"
    assert _pad_intact(wflat)


@pytest.mark.parametrize("G,K,M,N", lx.WGRAD_CASES)
def test_weight_gradient_kernel_is_bit_exact_on_integer_data(G, K, M, N):
    """cat_dense_wgrad + the chunk sum on operands in {-2..2}: ragged tiles, the element-wise loads of narrow heads and,
    at K = 5000, splits whose row range is empty (they must contribute zeros, not stale slabs)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    _premises(lx.wgrad_bounds(K))
    gen = torch.Generator(device="cuda").manual_seed(K + M + N)
    g64 = torch.randint(-2, 3, (G, K, M), generator=gen, device="cuda").double()
    x64 = torch.randint(-2, 3, (G, K, N), generator=gen, device="cuda").double()
    s64 = torch.randint(-lx.SLOT_MAX, lx.SLOT_MAX + 1, (G, M, N), generator=gen, device="cuda").double()
    want = torch.bmm(g64.transpose(1, 2), x64)
    S = ln.lib().cat_dense_wgrad_splits(G, K, M, N)
    rows_per = -(-(-(-K // S)) // 32) * 32
    if K == 5000:
        assert S * rows_per > K + rows_per, (S, rows_per)                        # trailing splits without rows exist
    assert lx.exact_equal(ln.dense_wgrad(g64.to(bf), x64.to(bf)), want)
    slot, flat = _strided((G, M, N), s64)
    ln.dense_wgrad(g64.to(bf), x64.to(bf), slot)
    torch.cuda.synchronize()
    assert lx.exact_equal(slot, s64 + want) and _pad_intact(flat)


@pytest.mark.parametrize("G,K,M,N0,N1", lx.WGRAD2_CASES)
def test_two_input_weight_gradient_is_bit_exact_on_integer_data(G, K, M, N0, N1):
    """cat_dense_wgrad with its second input (an LSTM layer's W_ih and W_hh) + cat_dense_sum_chunks2 into both slots."""
    from as_cops_and_thieves_amd import _learn_native as ln
    _premises(lx.wgrad_bounds(K))
    gen = torch.Generator(device="cuda").manual_seed(K + N0 + N1)
    g64 = torch.randint(-2, 3, (G, K, M), generator=gen, device="cuda").double()
    xs = [torch.randint(-2, 3, (G, K, n), generator=gen, device="cuda").double() for n in (N0, N1)]
    inits = [torch.randint(-lx.SLOT_MAX, lx.SLOT_MAX + 1, (G, M, n), generator=gen, device="cuda").double() for n in (N0, N1)]
    slots = [_strided((G, M, n), s) for n, s in zip((N0, N1), inits)]
    ln.dense_wgrad2(g64.to(bf), xs[0].to(bf), xs[1].to(bf), slots[0][0], slots[1][0])
    torch.cuda.synchronize()
    for (slot, flat), x, s in zip(slots, xs, inits):
        assert lx.exact_equal(slot, s + torch.bmm(g64.transpose(1, 2), x)) and _pad_intact(flat)


# ---------------------------------------------------------------------------------------------- convolutional trunk
def _trunk_run(c, x64, params64, d64, rows):
    from as_cops_and_thieves_amd import _learn_native as ln
    x = x64.to(bf)
    w1, b1, w2, b2 = (t.to(bf) for t in params64)
    block = 0 if c.rows is None else c.rows[1]
    out = ln.trunk_forward(x, w1, b1, w2, b2, c.R, rows, block)
    parts = ln.trunk_backward(x, w1, b1, w2, b2, out, d64.to(bf), c.R, rows, block)
    return out, parts


@pytest.mark.parametrize("c", lx.trunk_cases(), ids=lambda c: c.id)
def test_trunk_kernels_are_bit_exact_on_integer_data(c):
    """cat_trunk_forward / cat_trunk_backward / cat_trunk_grad_finish (new tensors and accumulated into row-strided slots)
    against fp64 autograd through the same two convolutions: the output and all four parameter gradients bit for bit.
    C in {2, 4}, R in {22, 64, 90, 102}, N in {1, 16, 17, 4099, 131 072}, and the in-place minibatch gather (x_rows) at
    the trainer's size (16 steps x 8192 of 32 768 sequences)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    seed = c.N + 10 * c.C + c.R
    params = lx.trunk_params(c, seed)
    _premises(lx.trunk_bounds(c, params[0], params[1], params[2]))
    z1 = lx.trunk_z1_max(params[0], params[1])
    x64, d64 = lx.trunk_inputs(c, seed, "cuda", z1)
    params = [t.cuda() for t in params]
    rows = None
    if c.rows is not None:
        rows = torch.randperm(c.rows[1], generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")[:c.rows[2]].contiguous()
    out_ref, grads_ref = lx.trunk_reference(c, lx.trunk_gather(c, x64, rows), *params, d64)
    out, parts = _trunk_run(c, x64, params, d64, rows)
    assert lx.exact_equal(out, out_ref), "forward"
    got = ln.trunk_grad_finish(parts, c.C, c.R)
    for name, gt, want in zip(("d_w1", "d_b1", "d_w2", "d_b2"), got, grads_ref):
        assert lx.exact_equal(gt, want), name
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    inits = [torch.randint(-lx.SLOT_MAX, lx.SLOT_MAX + 1, t.shape, generator=gen, device="cuda").double() for t in grads_ref]
    slots = [_strided(tuple(t.shape), s) for t, s in zip(grads_ref, inits)]
    ln.trunk_grad_finish(parts, c.C, c.R, tuple(s[0] for s in slots))
    torch.cuda.synchronize()
    for name, (slot, flat), s, want in zip(("d_w1", "d_b1", "d_w2", "d_b2"), slots, inits, grads_ref):
        assert lx.exact_equal(slot, s + want) and _pad_intact(flat), name + " into a slot"


def test_trunk_positions_no_second_window_covers_get_zero_gradient():
    """R = 90: the first convolution has 43 positions, the second one's windows (stride 3, width 5) cover 0..40 only.  The
    input is nonzero only on rays 87..89, which reach position 42 alone (and 89 no window at all): every dW1 entry must
    then be exactly 0, while the bias gradients (all positions) are still checked bit for bit."""
    from as_cops_and_thieves_amd import _learn_native as ln
    c = lx.TrunkCase(2, 4099, 4, 90)
    assert c.L1 == 43 and 3 * (c.L2 - 1) + 4 == 40
    params = lx.trunk_params(c, 5)
    x64, d64 = lx.trunk_inputs(c, 5, "cuda", lx.trunk_z1_max(params[0], params[1]))
    x64 = x64.view(c.G, c.N, c.C, c.R)
    x64[..., :87] = 0
    x64 = x64.reshape(c.G, c.N, c.C * c.R)
    params = [t.cuda() for t in params]
    out_ref, grads_ref = lx.trunk_reference(c, x64, *params, d64)
    assert float(grads_ref[0].abs().max()) == 0.0 and float(grads_ref[1].abs().max()) > 0
    out, parts = _trunk_run(c, x64, params, d64, None)
    got = ln.trunk_grad_finish(parts, c.C, c.R)
    torch.cuda.synchronize()
    assert lx.exact_equal(out, out_ref)
    assert float(got[0].float().abs().max()) == 0.0
    for gt, want in zip(got, grads_ref):
        assert lx.exact_equal(gt, want)


# ---------------------------------------------------------------------------------------------- GAE, sampler
@pytest.mark.parametrize("gamma,lam,T", lx.GAE_CASES)
def test_gae_scan_is_exact_on_integer_data(gamma, lam, T):
    """cat_ppo_gae_scan with integer rewards / values and gamma, lambda powers of two: every step of the recursion is exact
    in fp32, so advantages and returns equal the fp64 recursion exactly.  Dones at t = 0, at t = T - 1, in runs of
    consecutive ticks, on every tick of some columns, and at random."""
    from as_cops_and_thieves_amd import _learn_native as ln
    vmax = lx.GAE_VMAX
    assert lx.gae_bits(T, gamma, lam, vmax) <= 24
    G, N = 2, 777
    gen = torch.Generator(device="cuda").manual_seed(T)
    rew = torch.randint(-vmax, vmax + 1, (G, T, N), generator=gen, device="cuda").float()
    val = torch.randint(-vmax, vmax + 1, (G, T, N), generator=gen, device="cuda").float()
    last = torch.randint(-vmax, vmax + 1, (G, N), generator=gen, device="cuda").float()
    dones = torch.rand(T, N, generator=gen, device="cuda") < 0.2
    dones[:, :50] = False
    dones[0, :10] = True
    dones[T - 1, 10:20] = True
    dones[1:5, 20:30] = True
    dones[:, 30:40] = True
    want_adv, want_ret = lx.gae_reference(rew, val, dones, last, gamma, lam)
    assert torch.equal(want_adv.float().double(), want_adv) and torch.equal(want_ret.float().double(), want_ret)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    ln.ppo_gae(rew, val, dones, last, gamma, lam, adv, ret)
    torch.cuda.synchronize()
    assert torch.equal(adv, want_adv.float()) and torch.equal(ret, want_ret.float())


def _inverse_cdf(masses, u):
    """fp64: the number of prefix sums cdf_j (j < 3) with u * sum >= cdf_j ("u * sum >= cdf_j moves past j")."""
    cdf = torch.cumsum(masses, -1)
    return ((u.unsqueeze(-1) * cdf[..., -1:]) >= cdf[..., :3]).sum(-1)


def test_sampler_tie_convention_and_zero_mass_actions():
    """cat_rollout_sample on equal logits (masses exactly 1) and u in {0, 1/4, 1/2, 3/4, 1 - 2^-24}: the inverse CDF moves
    past action j when u * sum >= cdf_j.  Then one action's logit 200 below the others (its mass underflows to 0) at each
    of the four places: it is never drawn (the expected draws follow the same convention in fp64)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    us = torch.tensor(lx.UNIFORMS, dtype=torch.float64)
    rows_z, rows_u = [], []
    for zero in (None, 0, 1, 2, 3):
        for u in us:
            for base in (0.0, -3.5, 7.25):
                z = [base] * 4
                if zero is not None:
                    z[zero] = base - 200.0
                rows_z.append(z)
                rows_u.append(float(u))
    G, N = 2, len(rows_z)
    logits = torch.tensor(rows_z, dtype=torch.float64).to(bf).unsqueeze(0).repeat(G, 1, 1).cuda().contiguous()
    u = torch.tensor(rows_u, dtype=torch.float32).unsqueeze(0).repeat(G, 1).cuda().contiguous()
    masses = (logits.double() - logits.double().amax(-1, keepdim=True) > -100).double()      # 1, or 0 where the mass underflows
    want = _inverse_cdf(masses, u.double())
    act, logp = torch.empty(G, N, dtype=torch.int64, device="cuda"), torch.empty(G, N, device="cuda")
    actions = torch.full((N, 3), -1, dtype=torch.int32, device="cuda")
    ln.rollout_sample(logits, u, None, act, logp, None, actions, [2, 0])
    torch.cuda.synchronize()
    assert torch.equal(masses.gather(-1, act.unsqueeze(-1)).squeeze(-1), torch.ones_like(masses[..., 0])), "a zero-mass action was drawn"
    assert torch.equal(act, want)
    assert torch.equal(actions[:, 2].long(), act[0]) and torch.equal(actions[:, 0].long(), act[1]) and bool((actions[:, 1] == -1).all())
    want_logp = -torch.log(masses.sum(-1))
    assert torch.allclose(logp.double(), want_logp, rtol=0, atol=2e-6)
    equal = want[0, :15:3].tolist()
    assert equal == [0, 1, 2, 3, 3], equal                   # equal masses: the ties at u * 4 = 1, 2, 3 move past
