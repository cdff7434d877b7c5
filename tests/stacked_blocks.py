"""Per-block checks of the stacked networks' gradients: shared helpers of ``test_stacked_blocks_host.py`` (CPU) and
``test_gpu_stacked_blocks.py`` (GPU).  Importing this file needs no GPU.

``selfplay/stacked.py`` decides which buffer each kernel's gradient lands in (slots of the flat gradient buffer, the bias
sums riding in a weight-gradient launch, W_ih's gradient taken by the recurrence's backward, ...).  A fault there drops,
doubles or misplaces ONE parameter block while every kernel stays correct, so the checks here are per block:

    err(block) = |got - ref| / |ref|   (L2, ref = the per-agent reference module in fp64 on the CPU)

against ``3 * nu``, where nu is the worst block error of the yardstick -- the same reference module run by plain torch in
bf16 on the CPU (no kernel and no autograd Function of this project) -- for the same case and agent.  The kernels round
where a bf16 torch model rounds and accumulate in fp32, so they should sit at the yardstick's level; the factor 3 covers the
spread between two single noisy draws, and tying the bound to the WORST block covers blocks of 1..4 elements.  A block-level
fault gives an error of about 1, and ``3 * nu <= CAP = 0.5`` is asserted for every case on the CPU: the bound can never grow
into the region where it would hide half a block.
"""
from __future__ import annotations

import contextlib
import functools
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

from as_cops_and_thieves_amd import _learn_native
from as_cops_and_thieves_amd.selfplay.models import state_width
from as_cops_and_thieves_amd.selfplay.stacked import (HIDDEN, FlatParams, StackedNet, _module_for, _net_shapes, agent_state_dict,
                                                       init_from_modules, role_param_shapes)

FACTOR = 3.0     # block error bound = FACTOR * nu
CAP = 0.5        # FACTOR * nu must stay below this for every case and agent (a condition on the cases, not a measurement)
BF = torch.bfloat16


@dataclass(frozen=True)
class Spec:
    """One case of the shared list.  ``trunk``: the fused trunk kernels are expected to take the case (None: the net has no trunk);
    ``wgrad``: T * B reaches the weight-gradient kernels' threshold."""
    kind: str
    arch: str
    R: int
    G: int
    T: int
    B: int
    seed: int
    trunk: Optional[bool]
    wgrad: bool

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.arch}-R{self.R}-G{self.G}-T{self.T}-B{self.B}"

    @property
    def vwidth(self) -> Optional[int]:
        return state_width(3, 2, 64) if self.arch == "mlp" else None


def _pair(R, G, T, B, seed, trunk, wgrad):
    return [Spec(kind, "lstm", R, G, T, B, seed, trunk, wgrad) for kind in ("policy", "value")]


# the GPU test's cases; the host test checks FACTOR * nu <= CAP for each of them
CASES = (_pair(64, 3, 16, 32, 1, True, True)        # T * B = 512: wgrad / wgrad2 / bias_job kernels
         + _pair(64, 3, 16, 33, 2, True, True)      # 528 rows: not a tile multiple
         + _pair(64, 3, 4, 8, 3, True, False)       # 32 rows: baddbmm_ + sum_chunks route
         + _pair(32, 3, 16, 32, 4, True, True)      # fused trunk, L2 = 3
         + _pair(90, 3, 16, 32, 5, True, True)      # fused trunk, L2 = 13
         + _pair(128, 3, 16, 32, 6, False, True)    # the trunk kernels do not fit: Toeplitz-dense route
         + _pair(64, 1, 16, 32, 7, True, True)      # one agent
         + [Spec("policy", "mlp", 64, 3, 16, 32, 8, True, True),
            Spec("value", "mlp", 64, 3, 16, 32, 9, None, True)])   # no trunk, no LSTM; 778 inputs: not a multiple of 8
EXACT_CASES = tuple(s for s in CASES if s.R == 64 and s.G == 3 and s.B in (32, 8))   # the 512-row and the 32-row case of each kind


def _bf(t: torch.Tensor) -> torch.Tensor:
    """fp32 values that bf16 holds exactly."""
    return t.to(BF).to(torch.float32)


def make_case(kind: str, arch: str, R: int, G: int, T: int, B: int, seed: int, device, dtype) -> SimpleNamespace:
    """The inputs of one case, drawn on the CPU from ``seed`` (the same numbers on every device): a FlatParams whose master,
    compute copy and reference hold the same bf16-representable weights, and bf16-representable inputs, states and loss
    weights, so that every difference between two evaluations is arithmetic and none is input rounding."""
    vwidth = state_width(3, 2, 64) if arch == "mlp" else None
    fp = FlatParams(role_param_shapes(R, arch, vwidth), G, torch.device(device), dtype)
    init_from_modules(fp, R, [1000 * seed + 17 * g + 1 for g in range(G)], arch, vwidth)
    with torch.no_grad():
        fp.master.copy_(_bf(fp.master))
    fp.refresh()
    net = StackedNet(kind, R, fp, arch, vwidth)
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    n_out = 4 if kind == "policy" else 1
    x = _bf(torch.rand(G, T, B, net.in_width, generator=gen))
    h0, c0 = _bf(0.5 * rnd(net.layers, G, B, HIDDEN)), _bf(0.5 * rnd(net.layers, G, B, HIDDEN))
    keep = torch.ones(T, B)
    keep[0, 0::3] = 0.0                # some sequences restart at t = 0,
    keep[T // 2, 1] = 0.0              # one at a middle tick, the rest are carried
    # loss weights of one sign: the sums over the rows do not cancel, so a block's reference norm is not small against its terms
    # and agent g's scaled by 2^g: no block of one agent (the last bias is just the sum of r_out) equals another agent's
    pos = lambda *s: 0.5 + torch.rand(*s, generator=gen)
    scale = torch.exp2(torch.arange(G, dtype=torch.float32))
    r_out = _bf(pos(G, T, B, n_out)) * scale.view(G, 1, 1, 1)
    r_h, r_c = (_bf(0.25 * pos(net.layers, G, B, HIDDEN)) * scale.view(1, G, 1, 1) for _ in range(2))
    dev = lambda t: t.to(device)
    return SimpleNamespace(kind=kind, arch=arch, R=R, G=G, T=T, B=B, seed=seed, vwidth=vwidth, fp=fp, net=net, dtype=dtype, device=device,
                           x=dev(x), h0=dev(h0), c0=dev(c0), keep=dev(keep), r_out=dev(r_out), r_h=dev(r_h), r_c=dev(r_c),
                           blocks=list(_net_shapes(kind, R, arch, vwidth)))


def case_of(spec: Spec, device, dtype) -> SimpleNamespace:
    return make_case(spec.kind, spec.arch, spec.R, spec.G, spec.T, spec.B, spec.seed, device, dtype)


def run_stacked(case, with_state: bool, x=None, select=None, zero: bool = True):
    """Forward and backward of the case's StackedNet: the loss is sum(out * r_out) [+ sum(h_T * r_h) + sum(c_T * r_c)], its
    gradients (r_out, r_h, r_c: bf16-representable) reach the network exactly.  ``zero``: from a zeroed gradient buffer."""
    dt = case.dtype
    if zero:
        case.fp.grad.zero_()
    keep = case.keep if case.net.layers else None
    out, (h, c) = case.net.forward(case.x.to(dt) if x is None else x, (case.h0.to(dt), case.c0.to(dt)), keep, select=select)
    loss = (out.float() * case.r_out).sum()
    if with_state and case.net.layers:
        loss = loss + (h.float() * case.r_h).sum() + (c.float() * case.r_c).sum()
    loss.backward()
    return out.detach()


def reference_grads(case, g: int, dtype, with_state: bool = True) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """Agent g's network as the per-agent reference module (``models.py``) in ``dtype`` on the CPU, same loss.  Returns
    ({block name: gradient in fp64}, out [T, B, n_out] in fp64).  float64 is the reference, bfloat16 the yardstick."""
    m = _module_for(case.kind, case.R, case.arch, case.vwidth)
    m.load_state_dict(agent_state_dict(case.fp, g)[case.kind])
    m = m.to(dtype)
    x = case.x[g].cpu().to(dtype)
    T, B = case.T, case.B
    r_out = case.r_out[g].cpu().to(dtype)
    if case.arch == "mlp":
        out = m(x.reshape(T * B, -1)).reshape(T, B, -1)
        loss = (out * r_out).sum()
    else:
        starts = (case.keep.cpu() == 0)
        o, (hT, cT) = m(x.transpose(0, 1), (case.h0[:, g].cpu().to(dtype), case.c0[:, g].cpu().to(dtype)), starts.t())
        out = (o.unsqueeze(-1) if case.kind == "value" else o).transpose(0, 1)
        loss = (out * r_out).sum()
        if with_state:
            loss = loss + (hT * case.r_h[:, g].cpu().to(dtype)).sum() + (cT * case.r_c[:, g].cpu().to(dtype)).sum()
    loss.backward()
    return {n: q.grad.detach().double() for n, q in m.named_parameters()}, out.detach().double()


@functools.lru_cache(maxsize=None)
def _cached(spec: Spec, g: int, dtype, with_state: bool):
    return reference_grads(case_of(spec, "cpu", torch.float32), g, dtype, with_state)


def reference_of(spec: Spec, g: int, with_state: bool):
    """fp64 reference of a case of the shared list: computed once per process, shared by the tests, never modified."""
    return _cached(spec, g, torch.float64, with_state)


def yardstick_of(spec: Spec, g: int, with_state: bool):
    return _cached(spec, g, BF, with_state)


def _rel(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.double().reshape(-1).cpu(), ref.double().reshape(-1).cpu()
    return float((got - ref).norm() / ref.norm())


def block_errors(fp: FlatParams, kind: str, g: int, ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Per block |got - ref| / |ref| in fp64, ``got`` read out of the flat gradient buffer through ``fp.offsets``."""
    errs = {}
    for n, want in ref.items():
        off, k, _ = fp.offsets[f"{kind}.{n}"]
        assert k == want.numel(), n
        errs[n] = _rel(fp.grad[g, off:off + k], want)
    return errs


def yardstick_errors(spec: Spec, g: int, with_state: bool) -> Dict[str, float]:
    ref, yard = reference_of(spec, g, with_state)[0], yardstick_of(spec, g, with_state)[0]
    return {n: _rel(yard[n], ref[n]) for n in ref}


def noise(spec: Spec, g: int, with_state: bool = True) -> float:
    """nu: the yardstick's worst block error against fp64."""
    return max(yardstick_errors(spec, g, with_state).values())


def flat_of(fp: FlatParams, kind: str, grads: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The blocks laid out as one agent's row of the flat gradient buffer (fp64, zeros elsewhere)."""
    row = torch.zeros(fp.P, dtype=torch.float64)
    for n, v in grads.items():
        off, k, _ = fp.offsets[f"{kind}.{n}"]
        row[off:off + k] = v.reshape(-1)
    return row


def whole_vector_check(got: torch.Tensor, ref: torch.Tensor) -> bool:
    """The criterion of ``test_gpu_mappo.py::test_minibatch_step_in_bf16_on_gpu_matches_fp32_on_cpu`` on one agent's flat
    gradient: norm within 10 %, cosine > 0.98."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    ratio = float(got.norm() / ref.norm())
    cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()))
    return 0.9 < ratio < 1.1 and cos > 0.98


def padding_columns(fp: FlatParams) -> torch.Tensor:
    """[P] bool: the columns of the flat buffers that belong to no parameter."""
    pad = torch.ones(fp.P, dtype=torch.bool)
    for off, k, _ in fp.offsets.values():
        pad[off:off + k] = False
    return pad


def bf16_step(v: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 numbers at |v| (fp64; the smallest normal's spacing below it)."""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 7)


def format_table(spec: Spec, g: int, with_state: bool, got: Dict[str, float], ref: Dict[str, torch.Tensor]) -> str:
    yard = yardstick_errors(spec, g, with_state)
    nu = max(yard.values())
    lines = [f"{spec.id} agent {g} loss {'outputs+state' if with_state else 'outputs'}: nu = {nu:.4f}, bound = {FACTOR * nu:.4f}"]
    for n in ref:
        lines.append(f"  {n:32s} kernels {got[n]:.4f}  yardstick {yard[n]:.4f}  |ref| {float(ref[n].norm()):.4e}")
    return "\n".join(lines)


@contextlib.contextmanager
def record_routes():
    """Counts, while active, the calls ``selfplay/stacked.py`` makes into ``_learn_native`` on the gradient hand-over routes:
    yields a list of (function name, detail) in call order."""
    calls = []
    names = ("dense_wgrad", "dense_wgrad2", "sum_chunks", "trunk_grad_finish", "trunk_forward", "dense_forward", "dense_bias_act_")
    saved = {n: getattr(_learn_native, n) for n in names}

    def wrap(name, fn):
        def inner(*a, **kw):
            if name == "dense_wgrad":
                slot = a[2] if len(a) > 2 else kw.get("slot")
                job = a[3] if len(a) > 3 else kw.get("bias_job")
                detail = ("slot" if slot is not None else "return", "bias_job" if job is not None else "no_bias_job")
            elif name == "sum_chunks":
                dst = a[1] if len(a) > 1 else kw.get("dst")
                dst2 = a[2] if len(a) > 2 else kw.get("dst2")
                detail = ("return" if dst is None else "two_slots" if dst2 is not None else "slot",)
            elif name == "trunk_grad_finish":
                slots = a[3] if len(a) > 3 else kw.get("slots")
                detail = ("slots" if slots is not None else "return",)
            elif name == "trunk_forward":
                rows = a[6] if len(a) > 6 else kw.get("rows")
                detail = ("in_place" if rows is not None else "all_rows",)
            else:
                detail = ()
            calls.append((name,) + detail)
            return fn(*a, **kw)
        return inner
    try:
        for n, fn in saved.items():
            setattr(_learn_native, n, wrap(n, fn))
        yield calls
    finally:
        for n, fn in saved.items():
            setattr(_learn_native, n, fn)
