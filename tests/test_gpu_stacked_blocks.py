"""GPU: every parameter block's gradient of the stacked bf16 networks, block by block (``tests/stacked_blocks.py``).

The kernel tests (``test_gpu_{dense,lstm,trunk}_kernels.py``, ``test_gpu_learner_exact.py``) prove each kernel; their leaves carry
no pre-assigned ``.grad``, so they never take the routes by which ``selfplay/stacked.py`` hands a kernel's gradient to its slot of
the flat gradient buffer.  Here every case runs the whole ``StackedNet`` over a ``FlatParams`` and

  * asserts the route it took (which hand-overs ran, counted at the ``_learn_native`` boundary),
  * compares every block of every agent with the per-agent reference module in fp64: error <= 3 * nu, nu = the worst block
    error of plain torch bf16 on the CPU for the same case and agent (3 * nu <= 0.5 is asserted on the CPU for every case),
  * and checks, without a tolerance, what a misrouted block breaks: accumulation, determinism, padding columns, agent
    isolation, the bias pair, in-place minibatch selection, and the slot path against the return-a-tensor path.
"""
import warnings

import pytest
import torch

from tests import stacked_blocks as sb

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")
BF = torch.bfloat16

# Per-block exceptions to the 3 * nu bound: {(case id, block): (allowed multiple of nu, why the block is legitimately noisier)}.
# Empty: on the MI355X no block of any case needed more than 3 * nu (profiles/stacked_block_gradients.txt).
EXCEPTIONS = {}


def _losses(spec):
    return (False,) if spec.arch == "mlp" else (False, True)


def _count(calls, *key):
    return sum(1 for c in calls if c[:len(key)] == key)


def _expected_routes(spec, net):
    """What one forward + backward of the case must call, from ``selfplay/stacked.py``:
    fused trunk -> one trunk_grad_finish into four slots; features_extractor.5.weight is a permuted non-leaf view -> its weight
    gradient is RETURNED (and its bias sum goes to its slot by sum_chunks); every LSTM layer -> one sum_chunks into the b_ih and
    b_hh slots at once; at T * B >= 512 every LSTM layer's W_ih and W_hh gradients in one dense_wgrad2 and every head layer's
    weight gradient into its slot with the bias sum riding in the launch (bias_job); below, baddbmm_ into the slots (no kernel
    of ours) and one sum_chunks per bias."""
    has_trunk = spec.trunk is not None
    heads = net.n_head
    want = {("trunk_grad_finish", "slots"): 1 if spec.trunk else 0, ("trunk_grad_finish", "return"): 0,
            ("sum_chunks", "two_slots"): net.layers, ("sum_chunks", "return"): 0}
    if spec.wgrad:
        want.update({("dense_wgrad2",): net.layers, ("dense_wgrad", "slot", "bias_job"): heads, ("dense_wgrad", "slot", "no_bias_job"): 0,
                     ("dense_wgrad", "return", "no_bias_job"): 1 if has_trunk else 0, ("sum_chunks", "slot"): 1 if has_trunk else 0})
    else:
        want.update({("dense_wgrad2",): 0, ("dense_wgrad",): 0, ("sum_chunks", "slot"): heads + (1 if has_trunk else 0)})
    return want


def _assert_routes(spec, case, calls):
    from as_cops_and_thieves_amd import _learn_native as ln
    net, fp, N = case.net, case.fp, spec.T * spec.B
    if spec.trunk is not None:
        assert ln.trunk_supported(spec.G, N, net.C, spec.R) == spec.trunk
    assert ln.wgrad_supported(torch.empty(spec.G, N, 1), None) == spec.wgrad
    # the head layers' products: csrc/cat_dense.hip wherever the in-features are a multiple of 8 -- all but the non-recurrent
    # critic's first layer (778 inputs), which takes the library GEMM + dense_bias_act_
    lib_gemm = 0
    for j in range(net.n_head):
        w = fp.views[f"{spec.kind}.{net.head}.{2 * j}.weight"]
        ok = ln.gemm_supported(torch.empty(spec.G, 1, w.shape[2]), w)
        assert ok == (w.shape[2] % 8 == 0) and ok == (not (spec.arch == "mlp" and spec.kind == "value" and j == 0))
        lib_gemm += not ok
    assert _count(calls, "dense_bias_act_") == lib_gemm
    assert _count(calls, "dense_forward") == (1 if spec.trunk is not None else 0) + net.layers + net.n_head - lib_gemm
    for key, n in _expected_routes(spec, net).items():
        assert _count(calls, *key) == n, (spec.id, key, n, calls)


@pytest.mark.parametrize("spec", sb.CASES, ids=lambda s: s.id)
def test_every_block_of_every_agent_is_within_three_times_the_yardstick_noise_of_fp64(spec):
    case = sb.case_of(spec, "cuda", BF)
    failures = []
    for with_state in _losses(spec):      # outputs only = the production path (d_hT, d_cT arrive as None); outputs + final state
        with sb.record_routes() as calls:
            out = sb.run_stacked(case, with_state)
        torch.cuda.synchronize()
        _assert_routes(spec, case, calls)
        grad = case.fp.grad
        assert not bool(grad[:, sb.padding_columns(case.fp).to(grad.device)].any())
        for l in range(case.net.layers):    # the bias pair of a layer: one sum stored twice
            (o1, k, _), (o2, _, _) = (case.fp.offsets[f"{spec.kind}.lstm.bias_{n}_l{l}"] for n in ("ih", "hh"))
            assert torch.equal(grad[:, o1:o1 + k], grad[:, o2:o2 + k]) and bool(grad[:, o1:o1 + k].any())
        for g in range(spec.G):
            ref, out64 = sb.reference_of(spec, g, with_state)
            yard_out = sb.yardstick_of(spec, g, with_state)[1]
            nu = sb.noise(spec, g, with_state)
            errs = sb.block_errors(case.fp, spec.kind, g, ref)
            print(sb.format_table(spec, g, with_state, errs, ref))
            fwd = float((out[g].double().cpu() - out64).abs().max())
            fwd_bound = 3 * float((yard_out - out64).abs().max()) + 2.0 ** -8 * float(out64.abs().max())
            print(f"  forward: max error {fwd:.3e}, bound {fwd_bound:.3e}")
            if fwd > fwd_bound:
                failures.append((g, with_state, "forward", fwd, fwd_bound))
            for n, e in errs.items():
                factor = EXCEPTIONS.get((spec.id, n), (sb.FACTOR,))[0]
                if not e <= factor * nu:
                    failures.append((g, with_state, n, e, factor * nu))
    assert not failures, (spec.id, failures)


@pytest.mark.parametrize("spec", sb.EXACT_CASES, ids=lambda s: s.id)
def test_backward_is_deterministic_and_a_second_backward_adds_to_the_slots(spec):
    """Two passes from zeroed buffers give identical bits.  A second backward on top of the first gives, element by element, twice
    the single-pass value s to within one bf16 step: every slot computes rne(slot + r) from the fp32 sum r with |r - s| <= ulp(s) / 2,
    so the result is within ulp(s) / 2 of the representable 2 s.  A slot that overwrites gives s instead."""
    case = sb.case_of(spec, "cuda", BF)
    for with_state in _losses(spec):
        sb.run_stacked(case, with_state)
        once = case.fp.grad.clone()
        sb.run_stacked(case, with_state)
        assert torch.equal(case.fp.grad, once)
        sb.run_stacked(case, with_state, zero=False)
        twice = case.fp.grad.double()
        want = 2 * once.double()
        bad = (twice - want).abs() > sb.bf16_step(want)
        assert bool(once.any()) and not bool(bad.any()), (spec.id, with_state, _blocks_of(case.fp, bad))


def _blocks_of(fp, mask):
    """Names of the parameter blocks with a flagged column."""
    cols = mask.any(0).cpu()
    return [n for n, (off, k, _) in fp.offsets.items() if bool(cols[off:off + k].any())] + (["padding"] if bool(cols[sb.padding_columns(fp)].any()) else [])


@pytest.mark.parametrize("spec", sb.EXACT_CASES, ids=lambda s: s.id)
def test_padding_columns_stay_zero_through_backward_and_the_optimiser_step(spec):
    """Blocks start on 8-element boundaries and some are (4,), (1,) or (1, 64) long: a 16-byte store past a block's end lands in the
    padding.  No column outside every block may hold a gradient, and one optimiser step over the whole row leaves them zero."""
    from as_cops_and_thieves_amd import _learn_native as ln
    case = sb.case_of(spec, "cuda", BF)
    fp, G = case.fp, spec.G
    pad = sb.padding_columns(fp).to("cuda")
    assert int(pad.sum()) > 0 and not bool(fp.master[:, pad].any())
    sb.run_stacked(case, spec.arch != "mlp")
    assert not bool(fp.grad[:, pad].any())
    f32 = dict(dtype=torch.float32, device="cuda")
    ar = torch.zeros(G, fp.P + 1, **f32)
    ar[:, :-1].copy_(fp.grad)
    before = fp.master.clone()
    ln.ppo_adam_step(ar, torch.ones(G, fp.P, **f32), torch.ones(G, **f32), torch.zeros(G, fp.P, **f32), torch.zeros(G, fp.P, **f32),
                     torch.zeros(G, fp.P, **f32), fp.master, fp.lp, torch.zeros(G, **f32), torch.zeros(G, 256, **f32),
                     1e-3, 0.9, 0.999, 1e-8, 0.5, 0.0)
    torch.cuda.synchronize()
    assert not torch.equal(fp.master, before)
    assert not bool(fp.master[:, pad].any()) and not bool(fp.lp[:, pad].any())


@pytest.mark.parametrize("spec", sb.EXACT_CASES, ids=lambda s: s.id)
def test_another_agents_inputs_weights_and_loss_do_not_reach_an_agents_row(spec):
    a, b = sb.case_of(spec, "cuda", BF), sb.case_of(spec, "cuda", BF)
    with torch.no_grad():
        b.x[1] = b.x[1].flip(0).flip(1) * 0.5
        b.r_out[1] *= -0.75
        if b.net.layers:
            b.h0[:, 1] *= -1.0
            b.c0[:, 1] *= 0.5
            b.r_h[:, 1] *= 2.0
        b.fp.master[1] *= 1.125
    b.fp.refresh()
    with_state = spec.arch != "mlp"
    out_a, out_b = sb.run_stacked(a, with_state), sb.run_stacked(b, with_state)
    for g in (0, 2):
        assert torch.equal(out_a[g], out_b[g]) and torch.equal(a.fp.grad[g], b.fp.grad[g])
    assert not torch.equal(out_a[1], out_b[1]) and not torch.equal(a.fp.grad[1], b.fp.grad[1])


@pytest.mark.parametrize("kind", ["policy", "value"])
@pytest.mark.parametrize("R", [64, 90])
def test_minibatch_selected_in_place_gives_the_bits_of_the_gathered_copy(kind, R):
    """``forward(x_all, ..., select=idx)`` on a contiguous bf16 rollout buffer (the trunk kernels read the rows in place) against
    ``forward(x_all.index_select(2, idx), ...)``: identical outputs and identical bits in every block of the gradient buffer."""
    G, T, B_all, B = 3, 16, 48, 32
    case = sb.make_case(kind, "lstm", R, G, T, B, 11, "cuda", BF)
    x_all = sb.make_case(kind, "lstm", R, G, T, B_all, 12, "cuda", BF).x.to(BF).contiguous()
    idx = torch.randperm(B_all, generator=torch.Generator().manual_seed(13))[:B].to("cuda")
    results = []
    for in_place in (True, False):
        with sb.record_routes() as calls:
            if in_place:
                out = sb.run_stacked(case, True, x=x_all, select=idx)
            else:
                out = sb.run_stacked(case, True, x=x_all.index_select(2, idx))
        assert _count(calls, "trunk_forward", "in_place" if in_place else "all_rows") == 1 and _count(calls, "trunk_forward") == 1
        assert _count(calls, "trunk_grad_finish", "slots") == 1
        results.append((out.clone(), case.fp.grad.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert bool(results[0][1].any())


# ---------------------------------------------------------------------------------------------- slot path vs return path
def _leaves(shapes, G, seed, scale=0.1):
    """FlatParams leaves (gradient slots pre-assigned) and plain clones of them (no slot: the Functions return the gradients)."""
    from as_cops_and_thieves_amd.selfplay.stacked import FlatParams
    fp = FlatParams(shapes, G, torch.device("cuda"), BF)
    with torch.no_grad():
        fp.master.copy_((scale * torch.randn(G, fp.P, generator=torch.Generator().manual_seed(seed))).to("cuda") * fp.column_mask(""))
    fp.refresh()
    plain = {n: v.detach().clone().requires_grad_(True) for n, v in fp.views.items()}
    return fp, plain


def _rand(seed, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(BF).to("cuda")


def _assert_same_bits(fp, plain, name):
    assert torch.equal(fp.views[name].grad, plain[name].grad) and bool(plain[name].grad.any()), name


def _assert_one_step(fp, plain, name, g, x):
    """Two fp32 sums of the same K products in different orders, each rounded once to bf16: within one bf16 step, plus what
    reordering an fp32 sum can move it, K * 2^-23 * sum_k |g| |x| (matters only where the terms cancel)."""
    a, b = fp.views[name].grad.double(), plain[name].grad.double()
    K = g.shape[1]
    slack = K * 2.0 ** -23 * torch.bmm(g.double().abs().transpose(1, 2), x.double().abs())
    assert bool(((a - b).abs() <= sb.bf16_step(torch.maximum(a.abs(), b.abs())) + slack).all()) and bool(b.any()), name


@pytest.mark.parametrize("M,n_in,n_out,act", [(512, 128, 64, 1), (528, 64, 4, 0), (32, 128, 64, 1), (32, 64, 1, 0)])
def test_lin_act_slot_path_equals_the_return_path(M, n_in, n_out, act):
    """``_LinAct`` on FlatParams leaves and on plain clones.  From the code: the bias is the same chunk sum by the same kernel on both
    routes (alone, or riding in the weight gradient's launch), added to a zero slot or stored: identical bits.  The weight at
    M >= 512 is the same split-K slabs added up by the same kernel: identical bits.  Below 512 rows it is the library's
    ``baddbmm_`` into the slot against its ``bmm``: two roundings of possibly differently ordered fp32 sums, one bf16 step."""
    from as_cops_and_thieves_amd.selfplay.stacked import _LinAct
    G = 3
    fp, plain = _leaves({"w": (n_out, n_in), "b": (n_out,)}, G, seed=M + n_out)
    x, go = _rand(1, G, M, n_in), _rand(2, G, M, n_out)
    for leaves in (fp.views, plain):
        _LinAct.apply(x, leaves["w"], leaves["b"], act).backward(go)
    torch.cuda.synchronize()
    _assert_same_bits(fp, plain, "b")
    if M >= 512:
        _assert_same_bits(fp, plain, "w")
    else:
        _assert_one_step(fp, plain, "w", go, x)       # |go * act'| <= |go|
    assert not bool(fp.grad[:, sb.padding_columns(fp).to("cuda")].any())


@pytest.mark.parametrize("T,B", [(16, 32), (4, 8)])
def test_lstm_seq_slot_path_equals_the_return_path(T, B):
    """``_LSTMSeq`` without ``shared``.  The bias pair: one ``sum_chunks`` into both slots against one returned sum used twice --
    identical bits.  W_hh at T * B >= 512: ``dense_wgrad`` with the same splits on both routes -- identical bits; below, ``baddbmm_``
    against ``bmm``: one bf16 step."""
    from as_cops_and_thieves_amd.selfplay.stacked import HIDDEN, _LSTMSeq
    G, H = 3, HIDDEN
    fp, plain = _leaves({"w_hh": (4 * H, H), "b_ih": (4 * H,), "b_hh": (4 * H,)}, G, seed=T)
    h0, c0, r = _rand(3, G, B, H, scale=0.3), _rand(4, G, B, H, scale=0.5), _rand(5, G, T, B, H)
    keep = torch.ones(T, B, device="cuda")
    keep[T // 2, 1] = 0.0
    d_x = []
    for leaves in (fp.views, plain):
        xp = _rand(6, G, T, B, 4 * H).requires_grad_(True)
        out, hT, cT = _LSTMSeq.apply(xp, leaves["w_hh"], leaves["b_ih"], leaves["b_hh"], h0, c0, keep, None, True, None)
        out.backward(r)
        d_x.append(xp.grad)
    torch.cuda.synchronize()
    assert torch.equal(d_x[0], d_x[1])
    _assert_same_bits(fp, plain, "b_ih")
    _assert_same_bits(fp, plain, "b_hh")
    assert torch.equal(fp.views["b_ih"].grad, fp.views["b_hh"].grad)
    if T * B >= 512:
        _assert_same_bits(fp, plain, "w_hh")
    else:   # the saved h_in is h0 or an h = o * tanh(c): |h_in| <= max(1, |h0|)
        bound = torch.full((G, T * B, H), max(1.0, float(h0.abs().max())), device="cuda")
        _assert_one_step(fp, plain, "w_hh", d_x[0].reshape(G, T * B, 4 * H), bound)


def test_lstm_seq_with_shared_slot_path_equals_the_return_path():
    """The projection + recurrence pair of a layer.  On FlatParams leaves the recurrence's backward takes W_ih's gradient with its
    own in ONE ``dense_wgrad2`` launch and the projection's backward skips it; on plain clones each backward returns its own
    ``dense_wgrad``.  The split-K count of the joint launch is chosen for both widths together: where it equals the single
    launch's, the slabs are the same sums and the bits identical; where it differs, the fp32 partial sums are grouped differently
    and the results agree to one bf16 step."""
    from as_cops_and_thieves_amd import _learn_native as ln
    from as_cops_and_thieves_amd.selfplay.stacked import HIDDEN, _LinAct, _LSTMSeq, _SharedWgrad
    G, T, B, H, n_in = 3, 16, 32, HIDDEN, 256
    K = T * B
    fp, plain = _leaves({"w_ih": (4 * H, n_in), "w_hh": (4 * H, H), "b_ih": (4 * H,), "b_hh": (4 * H,)}, G, seed=9)
    inp, h0, c0, r = _rand(1, G, K, n_in), _rand(3, G, B, H, scale=0.3), _rand(4, G, B, H, scale=0.5), _rand(5, G, T, B, H)
    d_x, taken = [], []
    for leaves in (fp.views, plain):
        shared = _SharedWgrad()
        with sb.record_routes() as calls:
            xp = _LinAct.apply(inp, leaves["w_ih"], None, 0, shared)
            xp.retain_grad()
            out, hT, cT = _LSTMSeq.apply(xp.view(G, T, B, 4 * H), leaves["w_hh"], leaves["b_ih"], leaves["b_hh"], h0, c0, None, None, True, shared)
            out.backward(r)
        d_x.append(xp.grad)
        taken.append((shared.taken, _count(calls, "dense_wgrad2"), _count(calls, "dense_wgrad", "return")))
    torch.cuda.synchronize()
    assert taken == [(True, 1, 0), (False, 0, 2)]
    assert torch.equal(d_x[0], d_x[1])
    _assert_same_bits(fp, plain, "b_ih")
    _assert_same_bits(fp, plain, "b_hh")
    joint = ln.lib().cat_dense_wgrad_splits(G, K, 4 * H, 128 * (-(-n_in // 128) - (-H // 128)))
    for name, x, n in (("w_ih", inp, n_in), ("w_hh", None, H)):
        if ln.lib().cat_dense_wgrad_splits(G, K, 4 * H, n) == joint:
            _assert_same_bits(fp, plain, name)
        else:
            h_max = max(1.0, float(h0.abs().max()))            # the saved h_in is h0 or an h = o * tanh(c)
            _assert_one_step(fp, plain, name, d_x[0], x if x is not None else torch.full((G, K, H), h_max, device="cuda"))


@pytest.mark.parametrize("N,C,R", [(512, 4, 64), (32, 2, 64), (528, 2, 90)])
def test_conv_trunk_slot_path_equals_the_return_path(N, C, R):
    """``_ConvTrunk``: ``trunk_grad_finish`` adds the same slabs up in the same order and rounds the fp32 sum once on both routes
    (added to a zero slot, or stored): identical bits in all four blocks."""
    from as_cops_and_thieves_amd.selfplay.models import conv_out_len
    from as_cops_and_thieves_amd.selfplay.stacked import _ConvTrunk
    G = 3
    fp, plain = _leaves({"w1": (64, C, 5), "b1": (64,), "w2": (32, 64, 5), "b2": (32,)}, G, seed=N + R)
    x = torch.rand(G, N, C * R, generator=torch.Generator().manual_seed(2)).to(BF).to("cuda")
    go = _rand(3, G, N, conv_out_len(R) * 32)
    for leaves in (fp.views, plain):
        with sb.record_routes() as calls:
            _ConvTrunk.apply(x, leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], R).backward(go)
        assert _count(calls, "trunk_grad_finish", "slots" if leaves is fp.views else "return") == 1
    torch.cuda.synchronize()
    for name in ("w1", "b1", "w2", "b2"):
        _assert_same_bits(fp, plain, name)
    assert not bool(fp.grad[:, sb.padding_columns(fp).to("cuda")].any())
