"""Exact known-answer data for the learner kernels (csrc/cat_{dense,trunk,ppo,rollout}.hip): operand generators, fp64
references, the exactness premises and the comparison helpers.  Used by tests/test_gpu_learner_exact.py (on the GPU) and
tests/test_learner_exact_host.py (the premises and the helpers' teeth, on the CPU).  The LSTM window kernels (csrc/cat_lstm.hip)
have their exact cases in tests/lstm_exact.py (a saturating network forward, fabricated saved buffers backward), the fused act tick
(csrc/cat_act.hip) in tests/act_exact.py; ``lstm_reference`` and ``row_k`` below serve the bounded per-row test of long chains.

The idea: with small integer operands every bf16 product is exact, every fp32 partial sum is an integer below 2^24 (so
exact in ANY summation order and split), and every intermediate a kernel rounds to bf16 is an integer of magnitude
<= 256 (so that rounding changes nothing).  The kernel's bf16 result must then equal the fp64 result rounded once to
bf16 (round to nearest even) bit for bit, and a slot it accumulates into must equal (slot + exact) rounded once.

The premises are checked from the value RANGES of the generators (rigorous worst cases, not the drawn data), so a
later change of shapes or ranges that would make a case inexact fails on the CPU before it can make a GPU test flaky.
Sums are kept below 2^22 rather than 2^24: that margin covers accumulators that align addends to the largest exponent."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

BF16_INT = 256            # every integer of magnitude <= 256 is a bf16
SUM_LIMIT = 2 ** 22       # every partial sum of the exact cases stays below this
ACT_NONE, ACT_RELU = 0, 1
TRAIN_ROWS = 131072       # rows of one trainer minibatch: 4096 envs x 128 ticks / 16-tick windows = 32768 sequences / 4 minibatches x 16


# ---------------------------------------------------------------------------------------------- comparison helpers
def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16, round to nearest even (exact through fp32 for the integers these cases produce)."""
    assert x.dtype == torch.float64
    return x.to(torch.bfloat16)


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    """A truncating fp64 -> bf16 conversion (the defect the exact tests must reject)."""
    f = x.to(torch.float32)
    return (f.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def exact_equal(got: torch.Tensor, want64: torch.Tensor) -> bool:
    """got (bf16) equals the once-rounded fp64 result bit for bit."""
    w = rne_bf16(want64).to(got.device)
    return got.dtype == torch.bfloat16 and got.shape == w.shape and bool(torch.equal(got.view(torch.int16), w.view(torch.int16)))


def old_gemm_tolerance(got: torch.Tensor, want: torch.Tensor) -> bool:
    """tests/test_gpu_dense_kernels.py: |err| <= 2^-7 x max|want|."""
    return float((got.double() - want.double()).abs().max()) <= 2 ** -7 * float(want.abs().max())


def old_grad_tolerance(got: torch.Tensor, want: torch.Tensor) -> bool:
    """tests/test_gpu_trunk_kernels.py / test_gpu_lstm_kernels.py: relative L2 <= 2 %, cosine >= 0.999."""
    a, b = got.double().flatten(), want.double().flatten()
    err = float((a - b).norm() / b.norm().clamp_min(1e-12))
    cos = float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-12))
    return err <= 2e-2 and cos >= 0.999


def _ints(gen: torch.Generator, shape, lo: int, hi: int, device, zero_p: float = 0.0) -> torch.Tensor:
    """integers uniform in [lo, hi] as fp64, each forced to 0 with probability zero_p."""
    v = torch.randint(lo, hi + 1, shape, generator=gen, device=gen.device).double()
    if zero_p:
        v = v * (torch.rand(shape, generator=gen, device=gen.device) >= zero_p).double()
    return v.to(device)


# ---------------------------------------------------------------------------------------------- dense layers
@dataclass(frozen=True)
class DenseCase:
    """One layer: x [G, M, K] -> act(x w^T + b) [G, M, N].  ``signed``: operands in {-1, 0, 1} (many exact-zero
    pre-activations: the ReLU convention); else in {0, 1, 2} (large sums whose bf16 rounding is not exact)."""
    G: int
    M: int
    K: int
    N: int
    act: int
    signed: bool

    @property
    def vmax(self) -> int:
        return 1 if self.signed else 2

    @property
    def id(self) -> str:
        return f"G{self.G}-M{self.M}-K{self.K}-N{self.N}-{'relu' if self.act else 'none'}-{'signed' if self.signed else 'pos'}"


SLOT_MAX = 3              # the slots accumulated into start as integers in [-3, 3]


def dense_bounds(c: DenseCase) -> Dict[str, Tuple[int, int]]:
    """name -> (largest magnitude the case can reach, exactness limit)."""
    v = c.vmax
    return {
        "forward sum (x w + b)": (c.K * v * v + v, SUM_LIMIT),
        "act_grad output (bf16, feeds the GEMMs)": (v, BF16_INT),
        "bias gradient sum + slot": (c.M * v + SLOT_MAX, SUM_LIMIT),
        "input gradient sum": (c.N * v * v, SUM_LIMIT),
        "weight gradient sum + slot": (c.M * v * v + SLOT_MAX, SUM_LIMIT),
    }


def dense_data(c: DenseCase, seed: int, device) -> Dict[str, torch.Tensor]:
    """fp64 operands (all bf16-exact): x, w, b, d_y and the slots' starting values."""
    gen = torch.Generator(device=device).manual_seed(seed)
    lo, hi, zp = (-1, 1, 0.3) if c.signed else (0, 2, 0.0)
    return {"x": _ints(gen, (c.G, c.M, c.K), lo, hi, device, zp), "w": _ints(gen, (c.G, c.N, c.K), lo, hi, device, zp),
            "b": _ints(gen, (c.G, c.N), lo, hi, device), "d_y": _ints(gen, (c.G, c.M, c.N), lo, hi, device),
            "slot_w": _ints(gen, (c.G, c.N, c.K), -SLOT_MAX, SLOT_MAX, device),
            "slot_b": _ints(gen, (c.G, c.N), -SLOT_MAX, SLOT_MAX, device)}


def dense_reference(c: DenseCase, d: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """fp64: forward y, its bf16-stored value's ReLU mask (torch's threshold_backward: gradient where y > 0), the
    gradient g of the pre-activations, bias / input / weight gradients."""
    pre = torch.bmm(d["x"], d["w"].transpose(1, 2)) + d["b"].unsqueeze(1)
    y = torch.relu(pre) if c.act == ACT_RELU else pre
    y16 = rne_bf16(y).double()
    g = d["d_y"] * (y16 > 0).double() if c.act == ACT_RELU else d["d_y"]
    return {"prod": torch.bmm(d["x"], d["w"].transpose(1, 2)), "y": y, "y16": y16, "g": g, "db": g.sum(1),
            "dx": torch.bmm(g, d["w"]), "dw": torch.bmm(g.transpose(1, 2), d["x"])}


def net_layer_shapes():
    """(in, out, act) of every layer of _net_shapes (selfplay/stacked.py), both roles, R in {64, 90}: the trunk's flatten
    layer, the LSTM input / recurrent projections (bare products) and the heads (ReLU, the last one linear)."""
    from as_cops_and_thieves_amd.selfplay.stacked import _net_shapes
    out = set()
    for R in (64, 90):
        for kind in ("policy", "value"):
            s = _net_shapes(kind, R)
            n_head = sum(1 for n in s if n.startswith(f"{kind}_head.") and n.endswith(".weight"))
            for name, shp in s.items():
                if len(shp) != 2:
                    continue
                if name.startswith("features_extractor."):
                    out.add((shp[1], shp[0], ACT_RELU))
                elif name.startswith("lstm.weight"):
                    out.add((shp[1], shp[0], ACT_NONE))
                elif name.startswith(f"{kind}_head."):
                    j = int(name.split(".")[1]) // 2
                    out.add((shp[1], shp[0], ACT_NONE if j == n_head - 1 else ACT_RELU))
    return sorted(out)


def dense_cases():
    """Every net layer at the trainer's minibatch (G = 3 agents of a role), plus the ragged shapes of
    tests/test_gpu_dense_kernels.py.  ReLU layers get signed data, linear ones the positive flavour."""
    cases = [DenseCase(3, TRAIN_ROWS, k, n, act, act == ACT_RELU) for k, n, act in net_layer_shapes()]
    cases += [DenseCase(2, 1000, 64, 4, ACT_NONE, False), DenseCase(3, 777, 64, 1, ACT_NONE, False),
              DenseCase(1, 130, 72, 136, ACT_RELU, True), DenseCase(5, 300, 128, 64, ACT_RELU, True),
              DenseCase(2, 777, 128, 64, ACT_RELU, True), DenseCase(3, 4096, 64, 4, ACT_NONE, True)]
    return cases


# weight-gradient-only cases: (G, K rows, M, N) of tests/test_gpu_dense_kernels.py; K = 5000 leaves splits 32..38 empty
WGRAD_CASES = [(2, 5000, 64, 128), (1, 777, 128, 64), (2, 1000, 8, 8), (3, 4096, 136, 72), (3, 16384, 4, 64), (3, 16384, 1, 64),
               (2, 3000, 5, 12), (3, 16384, 512, 256)]
WGRAD_VMAX = 2
# the two-input weight gradient (an LSTM layer's W_ih and W_hh share d xproj): (G, K rows, M, N0, N1)
WGRAD2_CASES = [(3, TRAIN_ROWS, 512, 256, 128), (3, TRAIN_ROWS, 512, 128, 128), (2, 4099, 512, 128, 128), (1, 1024, 130, 72, 8)]


def wgrad_bounds(K: int, vmax: int = WGRAD_VMAX) -> Dict[str, Tuple[int, int]]:
    return {"weight gradient sum + slot": (K * vmax * vmax + SLOT_MAX, SUM_LIMIT)}


# ---------------------------------------------------------------------------------------------- convolutional trunk
@dataclass(frozen=True)
class TrunkCase:
    """_ConvTrunk on x [G, N, C * R]; ``rows`` = (steps, block, sel): the minibatch read in place out of a rollout buffer."""
    G: int
    N: int
    C: int
    R: int
    rows: Optional[Tuple[int, int, int]] = None

    @property
    def L1(self) -> int:
        return (self.R - 5) // 2 + 1

    @property
    def L2(self) -> int:
        return (self.L1 - 5) // 3 + 1

    @property
    def id(self) -> str:
        return f"G{self.G}-N{self.N}-C{self.C}-R{self.R}" + ("" if self.rows is None else "-rows{}x{}of{}".format(*self.rows))


def trunk_cases():
    cases = [TrunkCase(2 if N < 4099 else 1, N, C, R) for N in (1, 16, 17, 4099) for C in (2, 4) for R in (22, 64, 90, 102)]
    cases += [TrunkCase(1, TRAIN_ROWS, 2, 64), TrunkCase(1, TRAIN_ROWS, 4, 90), TrunkCase(3, TRAIN_ROWS, 4, 102),
              TrunkCase(1, TRAIN_ROWS, 4, 64, (16, 32768, 8192)), TrunkCase(3, 3 * 37, 4, 90, (3, 200, 37)),
              TrunkCase(2, 5 * 17, 2, 22, (5, 64, 17))]
    return cases


def trunk_params(c: TrunkCase, seed: int):
    """fp64 CPU w1 [G, 64, C, 5], b1 [G, 64], w2 [G, 32, 64, 5], b2 [G, 32], all in {-1, 0, 1}: the first layer's
    positive taps are sparse (P(1) = 1/6), so its ReLU output is often exactly 0 and stays small."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(c.G, 64, c.C, 5, generator=gen, dtype=torch.float64)
    w1 = (u < 1 / 6).double() - (u > 2 / 3).double()
    b1 = torch.randint(-1, 2, (c.G, 64), generator=gen).double()
    w2 = torch.randint(-1, 2, (c.G, 32, 64, 5), generator=gen).double()
    b2 = torch.randint(-1, 2, (c.G, 32), generator=gen).double()
    return w1, b1, w2, b2


def trunk_z1_max(w1: torch.Tensor, b1: torch.Tensor) -> int:
    """Largest first-layer output any input in {0, 1} can give: sum of the positive taps + the positive bias, per channel."""
    return int((w1.clamp_min(0).sum((2, 3)) + b1.clamp_min(0)).max())


def trunk_nnz(c: TrunkCase, z1_max: int) -> int:
    """Nonzero output-gradient entries per sample: as many as keep every weight-gradient sum below SUM_LIMIT."""
    per = max(5, z1_max)                                     # dW1 sums <= 5 |w2| |x| ||d_out||_1, dW2 sums <= max z1 ||d_out||_1
    return max(1, min(c.L2 * 32, (SUM_LIMIT - 1) // (c.N * per)))


def trunk_bounds(c: TrunkCase, w1, b1, w2) -> Dict[str, Tuple[int, int]]:
    z1 = trunk_z1_max(w1, b1)
    nnz = c.N * trunk_nnz(c, z1)                             # ||d_out||_1 (entries in {-1, 0, 1})
    return {
        "first-layer output (bf16 intermediate)": (z1, BF16_INT),
        "second-layer sum": (64 * 5 * z1 + 1, SUM_LIMIT),
        "d_z1 (bf16 intermediate): 2 covering windows x 32 channels": (2 * 32 * int(w2.abs().max()), BF16_INT),
        "dW1 / db1 sums": (5 * int(w2.abs().max()) * nnz, SUM_LIMIT),
        "dW2 sums": (max(z1, 1) * nnz, SUM_LIMIT),
        "db2 sums": (nnz, SUM_LIMIT),
        "slot + gradient": (max(5 * nnz, z1 * nnz) + SLOT_MAX, SUM_LIMIT),
    }


def trunk_inputs(c: TrunkCase, seed: int, device, z1_max: int):
    """x (fp64, {0, 1}) [G, rows of x, C * R] and d_out (fp64, {-1, 0, 1}) [G, N, L2 * 32] with trunk_nnz entries per sample."""
    gen = torch.Generator(device=device).manual_seed(seed)
    n_x = c.N if c.rows is None else c.rows[0] * c.rows[1]
    x = (torch.rand(c.G, n_x, c.C * c.R, generator=gen, device=device) < 0.5).double()
    cols, k = c.L2 * 32, trunk_nnz(c, z1_max)
    d = torch.zeros(c.G, c.N, cols, dtype=torch.float64, device=device)
    if k == cols:
        d = torch.randint(-1, 2, d.shape, generator=gen, device=device).double()
    else:
        idx = torch.randint(0, cols, (c.G, c.N, k), generator=gen, device=device)
        d.scatter_(2, idx, torch.randint(0, 2, idx.shape, generator=gen, device=device).double() * 2 - 1)
    return x, d


def trunk_gather(c: TrunkCase, x: torch.Tensor, rows: Optional[torch.Tensor]) -> torch.Tensor:
    if rows is None:
        return x
    steps, block, sel = c.rows
    return x.view(c.G, steps, block, -1).index_select(2, rows).reshape(c.G, steps * sel, -1)


def trunk_reference(c: TrunkCase, x, w1, b1, w2, b2, d_out):
    """fp64 autograd through Conv1d(C, 64, 5, 2) -> ReLU -> Conv1d(64, 32, 5, 3) -> ReLU written out as unfold + einsum
    (tests/test_gpu_trunk_kernels.py checks that formulation against F.conv1d).  x [G, N, C * R] (channel, ray) ->
    out [G, N, L2 * 32] (position, channel); returns out and the four parameter gradients for the output gradient d_out."""
    outs, grads = [], []
    for g in range(c.G):
        p = [t[g].detach().clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
        win = x[g].view(-1, c.C, c.R).unfold(2, 5, 2)
        z = torch.relu(torch.einsum("nclk,ock->nol", win, p[0]) + p[1].view(1, -1, 1))
        y = torch.relu(torch.einsum("nclk,ock->nol", z.unfold(2, 5, 3), p[2]) + p[3].view(1, -1, 1))
        out = y.transpose(1, 2).reshape(y.shape[0], -1)
        (out * d_out[g]).sum().backward()
        outs.append(out.detach())
        grads.append([t.grad for t in p])
    return torch.stack(outs), [torch.stack([gr[i] for gr in grads]) for i in range(4)]


# ---------------------------------------------------------------------------------------------- GAE, sampler
def gae_reference(rew, val, dones, last, gamma: float, lam: float):
    """fp64 textbook recursion (selfplay.mappo.compute_gae on doubles)."""
    from as_cops_and_thieves_amd.selfplay.mappo import compute_gae
    return compute_gae(rew.double(), val.double(), dones, last.double(), gamma, lam)


def gae_bits(T: int, gamma: float, lam: float, vmax: int) -> int:
    """Significant bits the recursion can need: integer part (sum of T deltas of at most 3 vmax) plus the fraction bits
    of the powers of gamma and gamma lambda (both powers of two here)."""
    import math
    frac = 0 if gamma == 1 and lam == 1 else int(round(-math.log2(gamma * lam))) * (T - 1) + int(round(-math.log2(gamma)))
    return (3 * vmax * T).bit_length() + frac


GAE_CASES = [(1.0, 1.0, 16), (1.0, 1.0, 128), (0.5, 0.5, 8), (0.5, 0.5, 3), (1.0, 1.0, 1)]     # (gamma, lambda, T)
GAE_VMAX = 3
UNIFORMS = (0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24)


# ---------------------------------------------------------------------------------------------- LSTM: per-row bounds
def lstm_reference(xproj, w_hh, h0, c0, keep):
    """nn.LSTM semantics step by step (gate order i f g o, state zeroed where keep == 0), in the dtype of the inputs
    (fp64 for the row bounds), autograd-differentiable.  xproj [G, T, B, 4H]; keep [T, B] or None."""
    G, T, B, _ = xproj.shape
    h, c = h0, c0
    outs = []
    for t in range(T):
        if keep is not None:
            k = keep[t].view(1, B, 1).to(h.dtype)
            h, c = h * k, c * k
        i, f, g, o = (xproj[:, t] + torch.bmm(h, w_hh.transpose(1, 2))).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs, 1), h, c


LSTM_ATOL = 2.0 ** -12    # of the whole tensor's largest magnitude: rows whose own scale is (nearly) zero


def row_k(got: torch.Tensor, want: torch.Tensor) -> float:
    """The smallest k with  max_row |got - want| <= k 2^-8 max_row |want| + LSTM_ATOL max |want|  for every row (last
    axis) -- what the per-row bound of the LSTM tests compares with its calibrated constant."""
    want = want.double()
    err = (got.double() - want).abs().amax(-1)
    scale = want.abs().amax(-1)
    atol = LSTM_ATOL * float(want.abs().max())
    return float(((err - atol).clamp_min(0) / (2.0 ** -8 * scale).clamp_min(1e-300)).max())
