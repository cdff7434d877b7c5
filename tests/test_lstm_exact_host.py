"""CPU: the premises of tests/test_gpu_lstm_exact.py, its coverage conditions, the tie of its references to the project's own
definition of the recurrence, the layout mirror and the teeth of its comparison (tests/lstm_exact.py).

1. Every case the GPU test runs meets, on its drawn data, the premises that make the kernel's right answer exactly known, and the
   coverage conditions that make the data able to see a defect.  Conditions that a case's T cannot meet are asked in the form it
   can: with T = 1 there is no tick after the first, so W_hh's sign flips are counted at t = 0 (h0 is nonzero there); chains of
   two steps exist from T = 2 (ending at even t) and T = 3 (at odd t) on, and only a chain gives narrow() something to round (a
   single step's products have at most 8 significant bits), so that share is asked from T = 2 on.
2. The forward reference without its roundings equals ``learner_exact.lstm_reference`` to 1e-12; the backward reference without its
   roundings, on saved values consistent with that forward pass, equals autograd through ``lstm_reference`` to 1e-10.
3. ``pack_saved`` / ``unpack_saved`` are inverses over all lanes, padding included, and the buffer sizes are the library's.
4. The twelve defects, emulated in torch, are each rejected by ``exact_equal`` on at least one case.

The gap this closes -- of the twelve, the earlier criterion (``learner_exact.old_grad_tolerance``: relative L2 <= 2 %, cosine >= 0.999
per tensor, as tests/test_gpu_lstm_kernels.py asks of d_xproj, d_w_hh, d_h0, d_c0 and d_bias) lets two through on that test's own kind
of data (``_old_admits``): truncating_narrow (a systematic bias of half a bf16 ulp in every gate gradient) and garbage_state_grads (no
tensor it looks at changes).  It sees the other ten only because they are gross here: row15_not_in_part drops a sixteenth of the
rows, where one row in 131 072 would pass any per-tensor tolerance (the bias-sum identity of test_gpu_lstm_kernels.py sees that one),
and part_without_row_ok shows only while the padding lanes hold something other than zeros.  ``ADMITTED_BY_OLD`` pins the list."""
import pytest

torch = pytest.importorskip("torch")

from tests import learner_exact as lx  # noqa: E402
from tests import lstm_exact as le  # noqa: E402

FWD, BWD = le.forward_cases(), le.backward_cases()
_F, _B = {}, {}


def fwd(c):
    if c.id not in _F:
        d = le.forward_data(c)
        _F[c.id] = (d, le.forward_reference(d))
    return _F[c.id]


def bwd(c):
    if c.id not in _B:
        d, track, stats = le.backward_data(c), {}, {}
        _B[c.id] = (d, le.backward_reference(d, track=track, stats=stats), track, stats)
    return _B[c.id]


def test_the_cases_reach_every_path_the_gpu_test_names():
    assert len({c.id for c in FWD}) == len(FWD) and len({c.id for c in BWD}) == len(BWD)
    assert {c.B for c in FWD} == {1, 15, 16, 17, 1381, 2725} and {c.T for c in FWD} == {1, 2, 7, 16}
    assert {c.biases for c in FWD} == {0, 1, 2} and {c.keep for c in FWD} == {None, "mask"} and any(c.strided for c in FWD)
    assert all(c.G <= 3 and c.T <= 16 for c in FWD + BWD)
    nb = le.blocks(le.FOLD_TRAIN.B)
    assert nb == 87 and nb * le.FOLD_TRAIN.G == 261 > 256 and le.FOLD_TRAIN.B % 16            # folds in two rounds, last block partial
    nb = le.blocks(le.FOLD_INFER.B)
    assert nb == 171 and nb * le.FOLD_INFER.G == 513 > 512
    assert le.HANDOVER in FWD and le.HANDOVER.biases == 0 and le.HANDOVER.B % 16
    assert float(le.forward_reference(le.forward_data(le.HANDOVER))["pre"].abs().min()) >= 35.9          # residues below e^-35.9
    assert {c.B for c in BWD} == {1, 16, 17, 33} and {c.T for c in BWD} == {1, 2, 7, 16}
    assert {(c.T, c.keep) for c in BWD if c.sets == "rich"} >= {(1, "free"), (2, "free"), (2, None), (16, "isolated"), (7, "isolated")}
    assert {(c.T, c.keep) for c in BWD if c.sets == "pow2"} == {(16, "runs2")}
    assert any(not c.d_out for c in BWD) and any(not c.d_last for c in BWD) and any(c.strided for c in BWD)
    assert all(c.T <= 2 for c in BWD if c.keep is None)


@pytest.mark.parametrize("c", FWD, ids=lambda c: c.id)
def test_forward_premises_and_coverage(c):
    d, ref = fwd(c)
    prem, cov = le.forward_premises(d, ref), le.forward_coverage(c, d, ref)
    for name, (value, limit, sense) in prem.items():
        print(f"{c.id}: premise  {name}: {value:.6g} ({sense} {limit:.6g})")
    for name, (value, least) in cov.items():
        print(f"{c.id}: coverage {name}: {value:.6g} (>= {least:.6g})")
    for name, (value, limit, sense) in prem.items():
        assert value >= limit if sense == ">=" else value <= limit, (name, value, limit)
    for name, (value, least) in cov.items():
        assert value >= least - 1e-9, (name, value, least)
    for k in ("xproj", "w_hh", "h0", "c0", "bias", "bias2"):                    # what goes to the kernel is held by bf16
        assert d[k] is None or torch.equal(le.narrow(d[k]), d[k]), k


@pytest.mark.parametrize("c", [c for c in FWD if c.biases and c.B <= 17], ids=lambda c: c.id)
def test_every_bias_vector_decides_gates(c):
    """A saturating network hides a small error of a pre-activation: the biases are large enough that each one, left out or read
    at a neighbouring index, changes at least a twentieth of the activated gates (hundreds of them in the smallest case)."""
    d, ref = fwd(c)
    for name in ("bias", "bias2")[:c.biases]:
        for what, other in (("left out", None), ("shifted by 16 units", torch.roll(d[name], 16, 1))):
            if other is None and name == "bias" and c.biases == 2:
                other = torch.zeros_like(d[name])                                   # bias2 needs a bias beside it
            bad = le.forward_reference({**d, name: other})
            changed = float((le.flush(bad["gates"]) != le.flush(ref["gates"])).double().mean())
            print(f"{c.id}: {name} {what}: {changed:.3f} of the gates change")
            assert changed >= 0.05 and not le.exact_equal(bad["out"].to(torch.bfloat16), ref["out"]), (name, what, changed)


@pytest.mark.parametrize("c", BWD, ids=lambda c: c.id)
def test_backward_premises_and_coverage(c):
    d, ref, track, stats = bwd(c)
    cov = le.backward_coverage(c, d, stats)
    for name, bits in track.items():
        print(f"{c.id}: premise  significant bits, {name}: {bits} (<= {le.BITS_LIMIT})")
    print(f"{c.id}: premise  longest chain: {le.longest_chain(d['keep'], c.T)} steps")
    for name, (value, least) in cov.items():
        print(f"{c.id}: coverage {name}: {value:.6g} (>= {least:.6g})")
    assert len(track) >= 7
    for name, bits in track.items():
        assert bits <= le.BITS_LIMIT, (name, bits)
    assert le.longest_chain(d["keep"], c.T) <= (3 if c.sets == "pow2" else 2)
    for name, (value, least) in cov.items():
        assert value >= least, (name, value, least)
    for k, v in d.items():
        assert v is None or torch.equal(le.narrow(v), v), k
    for k in ("d_xproj", "d_h0", "d_c0"):                                       # the outputs are what bf16 holds, part what fp32 holds
        assert torch.equal(le.narrow(ref[k]), ref[k]), k
    assert torch.equal(ref["part"].float().double(), ref["part"])
    # want_state_grads=False changes neither d_xproj nor part
    other = le.backward_reference(d, want_state=False)
    assert other["d_h0"] is None and other["d_c0"] is None
    assert torch.equal(other["d_xproj"], ref["d_xproj"]) and torch.equal(other["part"], ref["part"])


@pytest.mark.parametrize("with_keep", (False, True))
def test_the_references_are_the_projects_recurrence(with_keep):
    G, T, B = 2, 5, 19
    f, b = le.consistent_backward_data(G, T, B, seed=5, with_keep=with_keep)
    ref = le.forward_reference(f, rounding=False)
    leaves = [f[k].clone().requires_grad_(True) for k in ("xproj", "w_hh", "h0", "c0")]
    bias = (f["bias"] + f["bias2"]).clone().requires_grad_(True)
    out, hT, cT = lx.lstm_reference(leaves[0] + bias.view(G, 1, 1, -1), *leaves[1:], f["keep"])
    for name, got, want in (("out", ref["out"], out), ("h_T", ref["h_T"], hT), ("c_T", ref["c_T"], cT)):
        assert float((got - want.detach()).abs().max()) <= 1e-12, name
    ((out * b["d_out"]).sum() + (hT * b["d_hT"]).sum() + (cT * b["d_cT"]).sum()).backward()
    got = le.backward_reference(b, rounding=False)
    for name, g, want in (("d_xproj", got["d_xproj"], leaves[0].grad), ("d_h0", got["d_h0"], leaves[2].grad),
                          ("d_c0", got["d_c0"], leaves[3].grad), ("d_bias", got["part"].sum(1), bias.grad)):
        assert float((g - want).abs().max()) <= 1e-10, name
    # h_in is the operand of the weight gradient: d_w_hh = d_xproj^T h_in
    d_w = torch.einsum("gtbk,gtbh->gkh", got["d_xproj"], ref["h_in"])
    assert float((d_w - leaves[1].grad).abs().max()) <= 1e-10


@pytest.mark.parametrize("G,T,B", [(1, 1, 1), (3, 2, 17), (2, 16, 33), (3, 2, 1381)])
def test_the_layout_mirror(G, T, B):
    na, nc = le.saved_bytes(G, T, B)
    rows = le.blocks(B) * le.BM
    # the byte formulas of cat_lstm_saved_acts_bytes / cat_lstm_saved_cell_bytes: T G blocks NW (4 | 2) HH LANES 4 elements x 2 bytes
    assert na == T * G * le.blocks(B) * 8 * 4 * 1 * 64 * 4 * 2 and nc == T * G * le.blocks(B) * 8 * 2 * 1 * 64 * 4 * 2
    try:
        from as_cops_and_thieves_amd import _learn_native as ln
        sizes = ln.saved_sizes(G, T, B)
    except (OSError, RuntimeError) as e:            # no library here: the restated formulas above stand alone
        print("libcat_learn.so did not load:", e)
    else:
        assert sizes == (na, nc) and ln.HIDDEN == le.H
    la, lc = le.acts_layout(G, T, B), le.cell_layout(G, T, B)
    assert la.shape == (T, G, rows, 4, le.H) and lc.shape == (T, G, rows, 2, le.H)
    assert torch.equal(la.reshape(-1).sort().values, torch.arange(na // 2)) and torch.equal(lc.reshape(-1).sort().values, torch.arange(nc // 2))
    # a lane's four values are consecutive hidden units and consecutive elements; lanes r of a group are consecutive rows
    assert torch.equal(la[..., 1::4] - la[..., 0::4], torch.ones_like(la[..., 0::4])) and int(la[0, 0, 1, 0, 0] - la[0, 0, 0, 0, 0]) == 4
    assert int(la[0, 0, 0, 1, 0] - la[0, 0, 0, 0, 0]) == 256 and int(la[0, 0, 0, 0, 16] - la[0, 0, 0, 0, 0]) == 4 * 256
    gen = torch.Generator().manual_seed(B)
    gates = torch.randn(T, G, rows, 4, le.H, generator=gen).to(torch.bfloat16)
    cells = torch.randn(T, G, rows, 2, le.H, generator=gen).to(torch.bfloat16)
    acts_b, cell_b = le.pack_saved(gates, cells, B)
    assert acts_b.dtype == torch.uint8 and acts_b.numel() == na and cell_b.numel() == nc
    g2, c2 = le.unpack_saved(acts_b, cell_b, G, T, B)
    assert torch.equal(g2, gates) and torch.equal(c2, cells)
    a3, c3 = le.pack_saved(g2, c2, B)
    assert torch.equal(a3, acts_b) and torch.equal(c3, cell_b)
    # given the B valid rows only, the padding lanes are poisoned
    a4, c4 = le.pack_saved(gates[:, :, :B], cells[:, :, :B], B)
    g4, c5 = le.unpack_saved(a4, c4, G, T, B)
    assert torch.equal(g4[:, :, :B], gates[:, :, :B]) and bool(g4[:, :, B:].isnan().all()) and bool(c5[:, :, B:].isnan().all())


def test_the_comparison_rule():
    want = torch.tensor([1.0, 195 / 256, 0.0, 3.0, 4e-11], dtype=torch.float64)
    good = torch.tensor([1.0, 195 / 256, 4e-11, 3.0, 0.0]).to(torch.bfloat16)
    assert le.exact_equal(good, want)
    for i, v in ((1, 196 / 256), (2, 2.0 ** -24), (3, float("nan")), (0, 1.0 - 2.0 ** -8)):
        bad = good.clone()
        bad[i] = v
        assert not le.exact_equal(bad, want), i
    assert le.exact_equal(want.float(), want) and not le.exact_equal(None, want) and le.exact_equal(None, None)
    assert le.sig_bits(torch.tensor([0.0, 0.75, 5.0, 2.0 ** 20 + 2.0 ** -2])) == 23 and le.sig_bits(torch.zeros(3)) == 0
    a, w = torch.tensor([[[1.0, 0.5, 0.0]]], dtype=torch.float64), torch.tensor([[[1.0], [0.25], [8.0]]], dtype=torch.float64)
    assert le.sum_bits_bound(a, w) == 4                                         # terms 1 and 1/8: S = 9/8, unit 1/8


def _tensors(out):
    return {"d_xproj": out["d_xproj"], "d_h0": out["d_h0"], "d_c0": out["d_c0"], "part": out["part"]}


def _as_kernel(out):
    """What the kernel would hand back: bf16 gradients, fp32 part."""
    return {k: None if v is None else v.to(torch.float32 if k == "part" else torch.bfloat16) for k, v in _tensors(out).items()}


def _defect_runs(defect):
    """(case id, clean reference, defective outputs) over the cases: want_state_grads=False for the defect that only shows there."""
    want_state = defect != "garbage_state_grads"
    for c in BWD:
        d = bwd(c)[0]
        clean = bwd(c)[1] if want_state else le.backward_reference(d, want_state=False)
        yield c, clean, le.backward_reference(d, want_state=want_state, defect=defect)


# the defects the old criterion passes (computed by test_what_the_old_criterion_admits)
ADMITTED_BY_OLD = {"truncating_narrow", "garbage_state_grads"}


@pytest.mark.parametrize("defect", le.BWD_DEFECTS)
def test_a_backward_defect_is_rejected(defect):
    rejected = []
    for c, clean, bad in _defect_runs(defect):
        got = _as_kernel(bad)
        assert all(le.exact_equal(v, _tensors(clean)[k]) for k, v in _as_kernel(clean).items())          # the clean reference passes its own rule
        if not all(le.exact_equal(got[k], _tensors(clean)[k]) for k in got):
            rejected.append(c.id)
    print(f"{defect}: rejected on {len(rejected)} of {len(BWD)} cases")
    assert rejected, defect


def test_the_forward_defect_is_rejected():
    rejected = []
    for c in FWD:
        d, ref = fwd(c)
        bad = le.forward_reference(d, defect="h_in0_not_gated")
        assert le.exact_equal(ref["h_in"].to(torch.bfloat16), ref["h_in"])
        if not le.exact_equal(bad["h_in"].to(torch.bfloat16), ref["h_in"]):
            rejected.append(c.id)
    assert rejected and set(rejected) == {c.id for c in FWD if c.keep}


_OLD = {}


def _old_admits(defect) -> bool:
    """Would tests/test_gpu_lstm_kernels.py's per-tensor criterion pass a kernel with this defect?  On its own kind of data: free
    Gaussian operands (G = 2, T = 16, B = 100 with a partial last block, 30 % of the keep flags 0), the saved values of a forward
    pass over them, the kernel emulated WITH its bf16 roundings against the unrounded fp64 truth; d_xproj, d_h0, d_c0, the summed
    bias gradient and the weight gradient d_xproj^T h_in are each asked relative L2 <= 2 % and cosine >= 0.999."""
    if not _OLD:
        _OLD["data"] = f, b = le.consistent_backward_data(2, 16, 100, seed=3, with_keep=True)
        _OLD["truth"] = le.backward_reference(b, rounding=False)
        _OLD["h_in"] = le.forward_reference(f, rounding=False)["h_in"]
    f, b = _OLD["data"]
    if defect == "garbage_state_grads":
        return True                                 # no tensor of the old test changes: the buffers it writes do not exist
    bad = le.backward_reference(b, defect=defect if defect in le.BWD_DEFECTS else None)
    h_in = le.forward_reference(f, defect=defect if defect in le.FWD_DEFECTS else None)["h_in"]
    truth = _OLD["truth"]
    pairs = [(bad[k], truth[k]) for k in ("d_xproj", "d_h0", "d_c0")] + [(bad["part"].sum(1), truth["part"].sum(1))]
    pairs.append((torch.einsum("gtbk,gtbh->gkh", bad["d_xproj"], h_in), torch.einsum("gtbk,gtbh->gkh", truth["d_xproj"], _OLD["h_in"])))
    return all(lx.old_grad_tolerance(g, w) for g, w in pairs)


def test_what_the_old_criterion_admits():
    assert _old_admits(None)                        # the right kernel passes the old criterion
    admitted = {x for x in le.BWD_DEFECTS + le.FWD_DEFECTS if _old_admits(x)}
    print("the old criterion admits:", sorted(admitted))
    assert admitted == ADMITTED_BY_OLD
