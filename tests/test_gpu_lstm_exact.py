"""GPU: the LSTM window kernels of libcat_learn.so (csrc/cat_lstm.hip) held to answers that are exactly known (tests/lstm_exact.py;
tests/test_lstm_exact_host.py checks the premises and the coverage of every case used here, and that the comparison has teeth).

Forward, both instantiations (training: 8 waves, saved buffers; inference: 4 waves of 32 hidden units, nothing kept): a saturating
network whose out, h_T, c_T, h_in, activated gates, entering cell state and tanh of the leaving one are known bit for bit.  The saved
buffers are read through the Python mirror of the kernel's lane order, which this ties to the kernel.
Backward: ``seq_backward`` on FABRICATED saved buffers of dyadic values, chains cut by the keep mask so that every intermediate fits
fp32 exactly: d_xproj, d_h0, d_c0 and the fp32 per-block bias sums are known bit for bit.  The padding lanes of the last block hold
NaN.
Equality is bit for bit, magnitudes below 2^-24 in either value counting as 0 (residues of saturated gates)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import lstm_exact as le  # noqa: E402

FWD, BWD = le.forward_cases(), le.backward_cases()
_REF = {}


def _fwd_ref(c):
    if c.id not in _REF:
        d = le.forward_data(c)
        _REF[c.id] = (d, le.forward_reference(d))
    return _REF[c.id]


def _bwd_ref(c):
    if c.id not in _REF:
        d = le.backward_data(c)
        _REF[c.id] = (d, le.backward_reference(d))
    return _REF[c.id]


def _dev(x, dtype=torch.bfloat16):
    return None if x is None else x.to(dtype).cuda()


def _padded_view(x, fill):
    """x [G, T, B, W] as a view with padded outer strides into a buffer of ``fill`` (what a caller's slice gives)."""
    G, T, B, W = x.shape
    big = torch.full((G, T, B + 3, W + 8), fill, dtype=torch.bfloat16, device="cuda")
    big[:, :, 1:B + 1, 8:] = x
    return big[:, :, 1:B + 1, 8:]


def _forward(c, d, save, alias=False):
    from as_cops_and_thieves_amd import _learn_native as ln
    xproj = _dev(d["xproj"])
    if c.strided:
        xproj = _padded_view(xproj, 99.0)
    h0, c0 = _dev(d["h0"]), _dev(d["c0"])
    res = ln.seq_forward(xproj, _dev(d["w_hh"]), _dev(d["bias"]), h0, c0, _dev(d["keep"], torch.float32), save=save,
                         state_out=(h0, c0) if alias else None, bias2=_dev(d["bias2"]))
    torch.cuda.synchronize()
    if alias:
        assert res[1].data_ptr() == h0.data_ptr() and res[2].data_ptr() == c0.data_ptr()
    return res


def _check(name, got, want):
    assert got is not None and got.dtype in (torch.bfloat16, torch.float32), name
    assert le.exact_equal(got, want), (name, le.mismatches(got, want))


def _check_forward(c, ref, res, save):
    out, hT, cT, (h_in, acts, cell) = res
    for name, got in (("out", out), ("h_T", hT), ("c_T", cT)):
        assert got.dtype == torch.bfloat16
        _check(name, got, ref[name])
    if not save:
        assert h_in is None and acts is None and cell is None
        return
    _check("h_in", h_in, ref["h_in"])
    assert (acts.numel(), cell.numel()) == le.saved_bytes(c.G, c.T, c.B)
    gates, cells = le.unpack_saved(acts, cell, c.G, c.T, c.B)
    _check("saved_acts", gates[:, :, :c.B], ref["gates"])
    _check("saved_cell", cells[:, :, :c.B], ref["cells"])


@pytest.mark.parametrize("save", (True, False), ids=("train", "infer"))
@pytest.mark.parametrize("c", FWD, ids=lambda c: c.id)
def test_forward_equals_the_saturating_reference_bit_for_bit(c, save):
    d, ref = _fwd_ref(c)
    _check_forward(c, ref, _forward(c, d, save), save)


@pytest.mark.parametrize("c,save", [(le.FOLD_TRAIN, True), (le.FOLD_INFER, False), (le.FOLD_INFER, True)],
                         ids=("train-fold", "infer-fold", "train-at-the-infer-fold"))
def test_state_out_aliased_to_the_initial_state_changes_nothing(c, save):
    """The collector hands h0 / c0 themselves over as state_out: a workgroup reads its rows of the initial state before it writes
    the final one, also when it folds over several blocks."""
    d, ref = _fwd_ref(c)
    plain, aliased = _forward(c, d, save), _forward(c, d, save, alias=True)
    for name, a, b in zip(("out", "h_T", "c_T"), plain[:3], aliased[:3]):
        assert torch.equal(a, b), name
    if save:
        for name, a, b in zip(("h_in", "saved_acts", "saved_cell"), plain[3], aliased[3]):
            assert torch.equal(a, b), name
    _check_forward(c, ref, aliased, save)


def _backward(c, d, want_state=True, want_bias=True):
    from as_cops_and_thieves_amd import _learn_native as ln
    gates, cells = le.saved_of(d)
    acts, cell = le.pack_saved(gates, cells, c.B)                   # the padding lanes of the last block hold NaN
    if c.B % le.BM:
        g2, c2 = le.unpack_saved(acts, cell, c.G, c.T, c.B)
        assert bool(g2[:, :, c.B:].isnan().all()) and bool(c2[:, :, c.B:].isnan().all())
    d_out = _dev(d["d_out"])
    if c.strided:
        d_out = _padded_view(d_out, float("nan"))
    res = ln.seq_backward(d_out, _dev(d["d_hT"]), _dev(d["d_cT"]), _dev(d["w_hh"]), _dev(d["keep"], torch.float32), acts.cuda(), cell.cuda(),
                          (c.G, c.T, c.B), want_state_grads=want_state, want_bias_grad=want_bias)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("c", BWD, ids=lambda c: c.id)
def test_backward_on_fabricated_saved_buffers_bit_for_bit(c):
    d, ref = _bwd_ref(c)
    d_x, d_h0, d_c0, part = _backward(c, d)
    assert part.dtype == torch.float32 and part.shape == (c.G, le.blocks(c.B), 4 * le.H)
    for name, got in (("d_xproj", d_x), ("d_h0", d_h0), ("d_c0", d_c0), ("part", part)):
        assert not bool(got.isnan().any()), name                   # nothing of the poisoned padding lanes arrives
        _check(name, got, ref[name])
    # the final-state gradients not wanted: the last W_hh^T product is skipped, d_xproj and part do not change
    x2, h2, c2, p2 = _backward(c, d, want_state=False)
    assert h2 is None and c2 is None and torch.equal(x2, d_x) and torch.equal(p2, part)
    # the bias gradient not wanted
    x3, h3, c3, p3 = _backward(c, d, want_bias=False)
    assert p3 is None and torch.equal(x3, d_x) and torch.equal(h3, d_h0) and torch.equal(c3, d_c0)


def test_the_forward_kernels_saved_buffers_are_what_backward_takes():
    """The hand-over, once: the kernel's own saved buffers of a saturated case go into seq_backward.  Saturated gates have
    g (1 - g) = 0, so the reference has exact zeros in all of d_xproj and d_h0 and in much of d_c0; the kernel has residues there
    (|pre| >= 36 without biases: below e^-36 times the weights).  This shows that the real buffers are accepted; it tests no
    arithmetic."""
    from as_cops_and_thieves_amd import _learn_native as ln
    c = le.HANDOVER
    d, ref = _fwd_ref(c)
    out, hT, cT, (h_in, acts, cell) = _forward(c, d, True)
    gates, cells = le.flush(ref["gates"]).transpose(0, 1), le.flush(ref["cells"]).transpose(0, 1)
    gen = torch.Generator().manual_seed(1)
    b = {"gi": gates[:, :, :, 0], "gf": gates[:, :, :, 1], "gg": gates[:, :, :, 2], "go": gates[:, :, :, 3], "cin": cells[:, :, :, 0],
         "tc": cells[:, :, :, 1], "w_hh": d["w_hh"], "keep": d["keep"], "d_out": torch.randint(-3, 4, (c.G, c.T, c.B, le.H), generator=gen).double(),
         "d_hT": torch.randint(-2, 3, (c.G, c.B, le.H), generator=gen).double(), "d_cT": torch.randint(-2, 3, (c.G, c.B, le.H), generator=gen).double()}
    want = le.backward_reference(b)
    assert not bool(want["d_xproj"].any()) and not bool(want["d_h0"].any()) and bool(want["d_c0"].any())
    res = ln.seq_backward(_dev(b["d_out"]), _dev(b["d_hT"]), _dev(b["d_cT"]), _dev(d["w_hh"]), _dev(d["keep"], torch.float32), acts, cell,
                          (c.G, c.T, c.B), want_state_grads=True, want_bias_grad=True)
    torch.cuda.synchronize()
    for name, got, w in zip(("d_xproj", "d_h0", "d_c0", "part"), res, (want["d_xproj"], want["d_h0"], want["d_c0"], want["part"])):
        got = got.cpu().double()
        assert not bool(got.isnan().any()), name
        zero = w == 0
        assert bool(zero.any()) and float(got[zero].abs().max()) < le.ZERO_TOL, (name, float(got[zero].abs().max()))
