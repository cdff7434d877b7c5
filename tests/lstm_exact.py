"""Exact known-answer data for the LSTM window kernels (csrc/cat_lstm.hip: lstm_seq_fwd_kernel<true, 8>, <false, 4> and
lstm_seq_bwd_kernel): the cases, their generators, fp64 references that round where the kernels round, the premises the exactness
rests on, the coverage conditions, a Python mirror of the saved buffers' lane order and the comparison rule.  Used by
tests/test_gpu_lstm_exact.py (on the GPU) and tests/test_lstm_exact_host.py (premises, coverage, the tie to
``learner_exact.lstm_reference`` and the teeth, on the CPU).

Forward: a saturating network, as tests/act_exact.py builds one.  xproj and the biases are integers with 26 <= |x + b| <= 274
(``forward_data``: each of xproj, bias and bias2 decides the sign of a share of the gates), every row of W_hh holds one +-512 or
+-1024, h is a multiple of 2^-8 of magnitude <= 1 (0, or go tanh(n) stored as bf16: 195/256, 247/256, 255/256, 1), so W_hh h is 0
or of magnitude >= 390 and every gate pre-activation has |pre| >= 26 without it and >= 116 where it flips the sign.
The sigmoids are then within e^-26 of 0 or 1, tanh of the g gate within e^-52 of +-1, the cell state an integer plus
a residue below 1e-9, and tanh(n) lies at least 2^-10.1 from the nearest bf16 rounding boundary.  What this rests on and nobody has
measured: __expf and the hardware reciprocal within a few ulp (so that tanh_fast(n) lands within 2^-11 of tanh(n)) and residues below
2^-24.  Saturated gates leave such residues where the ideal value is 0 (bf16 can hold 4e-11), hence the comparison rule: bit equality
after magnitudes below 2^-24 are set to 0 in either value.

Backward: the kernel takes the saved buffers as inputs, so a test fabricates them in the kernel's lane order (``acts_layout`` /
``cell_layout``; the forward test ties that mirror to the kernel) from dyadic values: gi, go in {0, 1/4, 1/2, 3/4, 1}, gf in {0, 1/2,
1}, gg, tc in {0, +-1/2, +-1}, c_in in {-2 .. 2}, the incoming gradients small integers, W_hh with 8 nonzeros per row from {+-1/2,
+-1, +-2}.  The gradient of a long chain is not exact in fp32 for any operands (it decays through W_hh and meets fresh O(1) gradient
at every step), so the keep masks cut the chains: at most two consecutive steps with these "rich" sets, at most three with the
sigmoid gates in {0, 1/2, 1} ("pow2").  ``backward_reference(track=...)`` measures the significant bits of EVERY intermediate of the
drawn data, the running bias sums and a bound over every partial sum of the W_hh^T product included; the limit is 22 of fp32's 24.
Products of dyadic factors do not lose bits along the way, so contraction and association do not matter."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from tests import learner_exact as lx

H = 128
BM, NW, LANES = 16, 8, 64          # CAT_LSTM_ROWS_PER_BLOCK, the backward kernel's waves, lanes of a wave (HH = H / (16 NW) = 1)
ZERO_TOL = 2.0 ** -24
BITS_LIMIT = 22
MIN_SIGMOID_PRE, MIN_TANH_PRE = 24.0, 12.0
TANH_MARGIN = 2.0 ** -11
BWD_DEFECTS = ("kt_on_dc_only", "keep_of_next_tick", "row15_not_in_part", "part_without_row_ok", "one_minus_gg", "df_from_cell_out",
               "truncating_narrow", "d_out_of_next_tick", "d_c_last_ignored", "f_g_tiles_swapped", "garbage_state_grads")
FWD_DEFECTS = ("h_in0_not_gated",)


def blocks(B: int) -> int:
    return (B + BM - 1) // BM


# ---------------------------------------------------------------------------------------------- the layout mirror
def _lane_offset(B: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(block, wave, offset inside a 256-element tile) of row b < blocks(B) * 16 and hidden unit u: lane = 16 q + r holds the units
    16 w + 4 q .. + 3 of row 16 blk + r."""
    b = torch.arange(blocks(B) * BM).view(-1, 1)
    u = torch.arange(H).view(1, -1)
    lane = ((u % 16) // 4) * 16 + b % BM
    return (b // BM).expand(-1, H), (u // 16).expand(b.shape[0], -1), lane * 4 + u % 4


def acts_layout(G: int, T: int, B: int) -> torch.Tensor:
    """int64 [T, G, blocks(B) * 16, 4, H]: element offset of (t, g, b, gate i f g o, hidden unit) in saved_acts (acts_index of
    cat_lstm.hip with 8 waves, HH = 1).  Rows b >= B are the padding lanes of the last block."""
    blk, w, off = _lane_offset(B)
    tg = (torch.arange(T).view(T, 1) * G + torch.arange(G).view(1, G)).view(T, G, 1, 1, 1)
    gate = torch.arange(4).view(1, 1, 1, 4, 1)
    return (((tg * blocks(B) + blk.view(1, 1, -1, 1, H)) * NW + w.view(1, 1, -1, 1, H)) * 4 + gate) * (LANES * 4) + off.view(1, 1, -1, 1, H)


def cell_layout(G: int, T: int, B: int) -> torch.Tensor:
    """int64 [T, G, blocks(B) * 16, 2, H]: element offset of (t, g, b, which, hidden unit) in saved_cell; which 0 = the cell state
    entering the step, 1 = tanh of the one leaving it."""
    blk, w, off = _lane_offset(B)
    tg = (torch.arange(T).view(T, 1) * G + torch.arange(G).view(1, G)).view(T, G, 1, 1, 1)
    which = torch.arange(2).view(1, 1, 1, 2, 1)
    return (((tg * blocks(B) + blk.view(1, 1, -1, 1, H)) * NW + w.view(1, 1, -1, 1, H)) * 2 + which) * (LANES * 4) + off.view(1, 1, -1, 1, H)


def saved_bytes(G: int, T: int, B: int) -> Tuple[int, int]:
    """cat_lstm_saved_acts_bytes / cat_lstm_saved_cell_bytes restated: T G blocks NW (4 | 2) HH LANES 4 elements of 2 bytes."""
    n = T * G * blocks(B) * NW * LANES * 4 * 2
    return 4 * n, 2 * n


def pack_saved(gates: torch.Tensor, cells: torch.Tensor, B: int, pad: float = float("nan")) -> Tuple[torch.Tensor, torch.Tensor]:
    """gates [T, G, rows, 4, H], cells [T, G, rows, 2, H] (values bf16 holds; rows = B, or blocks(B) * 16 with the padding lanes
    given) -> the two saved buffers as uint8 tensors in the kernel's lane order.  Missing padding lanes are filled with ``pad``."""
    T, G, rows = gates.shape[:3]
    out = []
    for vals, lay in ((gates, acts_layout(G, T, B)), (cells, cell_layout(G, T, B))):
        if rows != lay.shape[2]:
            assert rows == B
            full = torch.full(lay.shape, pad, dtype=vals.dtype)
            full[:, :, :B] = vals
            vals = full
        flat = torch.empty(lay.numel(), dtype=torch.bfloat16)
        flat[lay.reshape(-1)] = vals.reshape(-1).to(torch.bfloat16)
        out.append(flat.view(torch.uint8))
    return out[0], out[1]


def unpack_saved(acts: torch.Tensor, cell: torch.Tensor, G: int, T: int, B: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The inverse: bf16 gates [T, G, blocks(B) * 16, 4, H] and cells [T, G, blocks(B) * 16, 2, H], padding lanes included."""
    return (acts.cpu().view(torch.bfloat16)[acts_layout(G, T, B)], cell.cpu().view(torch.bfloat16)[cell_layout(G, T, B)])


# ---------------------------------------------------------------------------------------------- comparison
def flush(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x.abs() < ZERO_TOL, torch.zeros_like(x), x)


def narrow(x: torch.Tensor, trunc: bool = False) -> torch.Tensor:
    """fp64 -> bf16 (round to nearest even, or the truncating defect) -> fp64: one narrow() of the kernel."""
    return (lx.trunc_bf16(x) if trunc else lx.rne_bf16(x)).double()


def exact_equal(got: Optional[torch.Tensor], want: Optional[torch.Tensor]) -> bool:
    """got (bf16 or fp32 from the kernel) against the fp64 reference: bit for bit in got's format, magnitudes below 2^-24 in either
    value counting as 0.  None only equals None (an output that must not exist); NaN equals nothing."""
    if got is None or want is None:
        return got is None and want is None
    g = got.detach().cpu()
    if g.dtype not in (torch.bfloat16, torch.float32) or g.shape != want.shape:
        return False
    w = want.to(g.dtype).double()                       # fp64 -> fp32 and fp64 -> bf16 both round to nearest even, once
    return bool(torch.equal(flush(g.double()), flush(w)))


def mismatches(got: torch.Tensor, want: torch.Tensor, limit: int = 8) -> str:
    """The first differing elements, for a failing assertion's message."""
    g, w = flush(got.detach().cpu().double()), flush(want.to(got.dtype).double())
    bad = ((g != w) | g.isnan()).nonzero()
    return f"{bad.shape[0]} of {g.numel()} differ: " + ", ".join(f"{tuple(i.tolist())}: got {float(g[tuple(i)])!r} want {float(w[tuple(i)])!r}"
                                                                   for i in bad[:limit])


def sig_bits(x: torch.Tensor) -> int:
    """The largest number of significant bits (highest to lowest set bit of the binary expansion) any element of fp64 x has."""
    m, _ = torch.frexp(x.double().abs().reshape(-1))
    mant = (m * 2.0 ** 53).to(torch.int64)
    mant = mant[mant != 0]
    if mant.numel() == 0:
        return 0
    low = (mant & -mant).double()
    return int(53 - torch.frexp(low)[1].min().item() + 1)


def _lsb_exp(x: torch.Tensor) -> torch.Tensor:
    """float32 exponent of the lowest set bit of every element of fp64 x (+inf where x is 0)."""
    m, e = torch.frexp(x.double().abs())
    mant = (m * 2.0 ** 53).to(torch.int64)
    low = torch.where(mant != 0, mant & -mant, torch.ones_like(mant)).double()
    tz = torch.frexp(low)[1] - 1
    return torch.where(mant != 0, (e - 53 + tz).float(), torch.full(x.shape, float("inf")))


def sum_bits_bound(a: torch.Tensor, w: torch.Tensor) -> int:
    """Significant bits ANY partial sum of sum_k a[g, b, k] w[g, k, m] can need, whatever the order: every term is a multiple of the
    element's smallest lowest-set-bit u, every partial sum at most S = sum |terms|, so it fits in floor(log2(S / u)) + 1 bits."""
    unit = (_lsb_exp(a).unsqueeze(-1) + _lsb_exp(w).unsqueeze(1)).amin(2)               # [G, B, M]; the lsb of a product is the product of the lsbs
    S = torch.bmm(a.abs(), w.abs())
    ok = S > 0
    if not bool(ok.any()):
        return 0
    return int((torch.floor(torch.log2(S[ok]) - unit[ok].double()) + 1).max().item())


# ---------------------------------------------------------------------------------------------- forward: cases, data, reference
@dataclass(frozen=True)
class FwdCase:
    """One window of G networks over B sequences.  keep: None or "mask" (0 at t = 0 on every other row, at the last tick on every
    third, at the interior tick T // 2 on every other, 20 % at random elsewhere); biases: 0, 1 or 2 vectors; strided: xproj is a
    padded view."""
    G: int
    T: int
    B: int
    keep: Optional[str]
    biases: int
    strided: bool = False

    @property
    def seed(self) -> int:
        return 100000 * self.G + 10 * self.B * 17 + self.T + (7 if self.keep else 0) + 1000 * self.biases

    @property
    def id(self) -> str:
        return f"G{self.G}-T{self.T}-B{self.B}-{'keep' if self.keep else 'nokeep'}-bias{self.biases}" + ("-strided" if self.strided else "")


FOLD_TRAIN = FwdCase(3, 2, 1381, "mask", 2)     # nb = 87, nb G = 261 > 256: the training launch folds in two rounds, last block partial
FOLD_INFER = FwdCase(3, 1, 2725, "mask", 1)     # nb = 171, nb G = 513 > 512: the inference launch folds


HANDOVER = FwdCase(3, 7, 17, "mask", 0)         # the one case whose own saved buffers go into backward: no biases, so |pre| >= 36


def forward_cases() -> List[FwdCase]:
    return [FwdCase(1, 1, 1, None, 0), FwdCase(2, 16, 1, "mask", 1), FwdCase(2, 1, 15, "mask", 2), FwdCase(2, 7, 15, None, 1, True),
            FwdCase(3, 2, 16, "mask", 0), FwdCase(1, 16, 16, None, 2), FwdCase(2, 7, 17, "mask", 2, True), FwdCase(3, 16, 17, "mask", 1),
            FwdCase(1, 1, 17, None, 0), FwdCase(2, 2, 17, "mask", 2), FOLD_TRAIN, FOLD_INFER, FwdCase(3, 2, 2725, None, 0), HANDOVER]


H_VALUES = (0.0, 255 / 256, -255 / 256, 195 / 256, -195 / 256, 247 / 256, -247 / 256, 1.0, -1.0)     # of h0: multiples of 2^-8
GATE_POS = (0.6, 0.5, 0.5, 0.7)                 # share of positive xproj in the blocks i, f, g, o (h = go tanh c is else too often 0)


def _choice(gen: torch.Generator, values, shape) -> torch.Tensor:
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def forward_data(c: FwdCase) -> Dict[str, Optional[torch.Tensor]]:
    """fp64 CPU operands, all bf16-exact integers.  Without a bias: |xproj| in 36 .. 50.  With one: |xproj| in 28 .. 32 or 88 .. 92
    and |bias| in 58 .. 62, so the bias decides a gate's sign where xproj is small and xproj where it is large -- a bias read at a
    wrong index, or left out, flips gates -- and |x + b| lies in 26 .. 34, 86 .. 94 or 146 .. 154.  With two: |bias| in 119 .. 121 and
    |bias2| in 59 .. 61, their sum near +-60 or +-180, |x + b| in 26 .. 274.  w_hh [G, 4H, H] has one +-512 or +-1024 per row (W_hh h
    is 0 or at least 390 in magnitude), h0 is from H_VALUES, c0 integers in -2 .. 2, keep [T, B]."""
    gen = torch.Generator().manual_seed(c.seed)
    G, T, B = c.G, c.T, c.B
    pos = torch.tensor(GATE_POS, dtype=torch.float64).repeat_interleave(H)

    def signs(shape):
        return (torch.rand(shape, generator=gen, dtype=torch.float64) < pos).double() * 2 - 1

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=gen).double()
    shape = (G, T, B, 4 * H)
    if c.biases == 0:
        xproj = signs(shape) * ints(36, 50, shape)
    else:
        large = (torch.rand(shape, generator=gen) < 0.5).double()
        xproj = signs(shape) * (ints(28, 32, shape) + 60 * large)
    w = torch.zeros(G, 4 * H, H, dtype=torch.float64)
    col = torch.randint(0, H, (G, 4 * H, 1), generator=gen)
    w.scatter_(2, col, _choice(gen, (512.0, -512.0, 1024.0, -1024.0), (G, 4 * H, 1)))
    d = {"xproj": xproj, "w_hh": w, "h0": _choice(gen, H_VALUES, (G, B, H)), "c0": ints(-2, 2, (G, B, H)), "bias": None, "bias2": None, "keep": None}
    if c.biases == 1:
        d["bias"] = signs((G, 4 * H)) * ints(58, 62, (G, 4 * H))
    if c.biases == 2:
        d["bias"] = signs((G, 4 * H)) * ints(119, 121, (G, 4 * H))
        d["bias2"] = (ints(0, 1, (G, 4 * H)) * 2 - 1) * ints(59, 61, (G, 4 * H))
    if c.keep:
        keep = (torch.rand(T, B, generator=gen) > 0.2).double()
        keep[0, ::2] = 0.0
        keep[T - 1, ::3] = 0.0
        if T >= 3:
            keep[T // 2, ::2] = 0.0
        d["keep"] = keep
    return d


def forward_reference(d: Dict[str, Optional[torch.Tensor]], rounding: bool = True, defect: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """fp64, rounding where the kernel does: h is narrowed before it enters the next step's product and h_in; out, h_T, c_T and the
    saved values are narrowed on store; the two bias vectors are summed and rounded once; the cell state stays unrounded across the
    window.  Returns out [G, T, B, H], h_T, c_T, h_in [G, T, B, H], gates [T, G, B, 4, H] (activated i f g o), cells [T, G, B, 2, H]
    (c entering the step, tanh c leaving it) as the kernel stores them, and -- unrounded, for the premises -- pre [T, G, B, 4, H]
    with and pre_x without the recurrent term and c_out [T, G, B, H].  rounding=False: the plain recurrence."""
    assert defect in (None,) + FWD_DEFECTS
    nar = narrow if rounding else (lambda x: x)
    x, w = d["xproj"], d["w_hh"]
    G, T, B, _ = x.shape
    keep = d["keep"]
    bsum = torch.zeros(G, 4 * H, dtype=torch.float64)
    if d["bias"] is not None:
        bsum = nar(d["bias"] + (d["bias2"] if d["bias2"] is not None else 0.0))
    k0 = keep[0].view(1, B, 1) if keep is not None else 1.0
    h, c = nar(d["h0"] * k0), d["c0"] * k0
    h_first = nar(d["h0"]) if defect == "h_in0_not_gated" else h
    out, h_in, gates, cells, pres, pres_x, c_outs = [], [], [], [], [], [], []
    for t in range(T):
        h_in.append(h_first if t == 0 else h)
        base = x[:, t] + bsum.view(G, 1, -1)
        pre = base + torch.bmm(h, w.transpose(1, 2))
        pi, pf, pg, po = pre.chunk(4, dim=-1)
        gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
        cy = gf * c + gi * gg
        tc = torch.tanh(cy)
        hy = go * tc
        out.append(nar(hy))
        gates.append(torch.stack([nar(gi), nar(gf), nar(gg), nar(go)], 2))
        cells.append(torch.stack([nar(c), nar(tc)], 2))
        pres.append(pre.view(G, B, 4, H)); pres_x.append(base.view(G, B, 4, H)); c_outs.append(cy)
        if t + 1 < T:
            kn = keep[t + 1].view(1, B, 1) if keep is not None else 1.0
            h, c = nar(hy * kn), cy * kn
    return {"out": torch.stack(out, 1), "h_T": nar(hy), "c_T": nar(cy), "h_in": torch.stack(h_in, 1), "gates": torch.stack(gates),
            "cells": torch.stack(cells), "pre": torch.stack(pres), "pre_x": torch.stack(pres_x), "c_out": torch.stack(c_outs)}


def _bf16_boundary_distance(y: torch.Tensor) -> torch.Tensor:
    """Distance of y from the nearest midpoint between two neighbouring bf16 values (where its rounding would change)."""
    f = y.float()
    lo = (f.view(torch.int32) & -65536).view(torch.float32).double()          # truncation: the bf16 at or below |y| in magnitude
    ulp = torch.ldexp(torch.ones_like(lo), torch.frexp(lo.abs().clamp_min(1e-300))[1] - 8)
    return ((y.double() - lo).abs() - ulp / 2).abs()


def forward_premises(d, ref) -> Dict[str, Tuple[float, float, str]]:
    """name -> (value, limit, ">=" or "<="), on the drawn data."""
    pre = ref["pre"]
    sig = pre[:, :, :, [0, 1, 3]].abs().min()
    c_all = torch.cat([ref["c_out"].reshape(-1), ref["cells"][:, :, :, 0].reshape(-1)])
    frac = (c_all - c_all.round()).abs().max()
    reach = ref["c_out"].round()
    nz = reach[reach != 0]
    dist = _bf16_boundary_distance(torch.tanh(nz)).min() if nz.numel() else torch.tensor(1.0)
    hmul = (flush(ref["h_in"]) * 256 - (flush(ref["h_in"]) * 256).round()).abs().max()
    return {"min |pre| of the sigmoid gates": (float(sig), MIN_SIGMOID_PRE, ">="),
            "min |pre| of the g gate": (float(pre[:, :, :, 2].abs().min()), MIN_TANH_PRE, ">="),
            "cell state: distance from an integer": (float(frac), 2.0 ** -30, "<="),
            "max |cell state| (an integer bf16 holds)": (float(c_all.abs().max()), 256.0, "<="),
            "tanh(cell): distance from a bf16 rounding boundary": (float(dist), TANH_MARGIN, ">="),
            "h: distance from a multiple of 2^-8": (float(hmul), 0.0, "<=")}


def forward_coverage(c: FwdCase, d, ref) -> Dict[str, Tuple[float, float]]:
    """name -> (share or count, least allowed)."""
    cov = {}
    g = flush(ref["gates"])
    for j, name in enumerate("ifgo"):
        hi = float((g[:, :, :, j] == 1).double().mean())
        lo_v = -1.0 if name == "g" else 0.0
        lo = float((g[:, :, :, j] == lo_v).double().mean())
        cov[f"gate {name} at its high value"] = (hi, 0.2)
        cov[f"gate {name} at its low value"] = (lo, 0.2)
        cov[f"gate {name} saturated"] = (hi + lo, 1.0 - 1e-9)
    cov["h nonzero"] = (float((flush(ref["out"]) != 0).double().mean()), 0.3)
    flip = ((ref["pre"] > 0) != (ref["pre_x"] > 0)).any(3)                      # [T, G, B, H]: some gate's sign changed by W_hh h
    sel = flip[1:] if c.T >= 2 else flip
    cov["W_hh changes a gate's sign" + (" (t >= 1)" if c.T >= 2 else " (t = 0)")] = (float(sel.double().mean()), 0.1)
    if d["keep"] is not None:
        k = d["keep"]
        cov["keep = 0 at t = 0"] = (float((k[0] == 0).sum()), 1)
        cov["keep = 1 at t = 0"] = (float((k[0] == 1).sum()), 1 if c.B > 1 else 0)
        if c.T >= 2:
            cov["keep = 0 at the last tick"] = (float((k[-1] == 0).sum()), 1)
        if c.T >= 3:
            cov["keep = 0 at an interior tick"] = (float((k[1:-1] == 0).sum()), 1)
    return cov


# ---------------------------------------------------------------------------------------------- backward: cases, data, reference
@dataclass(frozen=True)
class BwdCase:
    """keep: None, "free" (T <= 2: independent coin flips), "isolated" (no two consecutive ones: chains of two steps) or "runs2"
    (runs of at most two ones: chains of three).  sets: "rich" or "pow2" (the sigmoid gates in {0, 1/2, 1}).  d_out / d_last:
    whether those gradients are given (else None = 0); strided: d_out is a padded view."""
    G: int
    T: int
    B: int
    keep: Optional[str]
    sets: str = "rich"
    d_out: bool = True
    d_last: bool = True
    strided: bool = False

    @property
    def seed(self) -> int:
        return 100000 * self.G + 1000 * self.T + 10 * self.B + {None: 0, "free": 1, "isolated": 2, "runs2": 3}[self.keep]

    @property
    def id(self) -> str:
        return (f"G{self.G}-T{self.T}-B{self.B}-{self.keep or 'nokeep'}-{self.sets}" + ("" if self.d_out else "-no_d_out")
                + ("" if self.d_last else "-no_d_last") + ("-strided" if self.strided else ""))


def backward_cases() -> List[BwdCase]:
    return [BwdCase(3, 1, 1, "free"), BwdCase(2, 2, 16, "free"), BwdCase(2, 2, 17, None), BwdCase(3, 1, 33, None),
            BwdCase(2, 16, 17, "isolated"), BwdCase(2, 7, 33, "isolated"), BwdCase(1, 7, 16, "isolated", strided=True),
            BwdCase(2, 16, 33, "runs2", "pow2"), BwdCase(3, 16, 1, "runs2", "pow2"),
            BwdCase(2, 2, 17, "free", d_out=False), BwdCase(2, 7, 33, "isolated", d_last=False), BwdCase(2, 2, 16, "free", strided=True)]


def _keep_mask(form: Optional[str], T: int, B: int, gen: torch.Generator) -> Optional[torch.Tensor]:
    """keep[t] = 1 lets dh and dc pass from step t to step t - 1 (keep[0]: into d_h0 / d_c0); a run of n ones is a chain of n + 1
    steps, the last of which may be the hand-over to d_h0 / d_c0."""
    if form is None:
        return None
    keep = (torch.rand(T, B, generator=gen) < 0.5).double()
    if form == "free":
        assert T <= 2
        return keep
    longest = {"isolated": 1, "runs2": 2}[form]
    for b in range(B):
        run = 0
        for t in range(T):
            run = run + 1 if keep[t, b] else 0
            if run > longest:
                keep[t, b], run = 0.0, 0
    return keep


def longest_chain(keep: Optional[torch.Tensor], T: int) -> int:
    """Steps of the longest chain the gradient runs through."""
    if keep is None:
        return T
    best = 1
    for b in range(keep.shape[1]):
        run = 1
        for t in range(1, T):
            run = run + 1 if keep[t, b] else 1
            best = max(best, run)
    return best


def backward_data(c: BwdCase) -> Dict[str, Optional[torch.Tensor]]:
    """fp64 CPU: fabricated saved values gi gf gg go cin tc [G, T, B, H], d_out [G, T, B, H], d_hT, d_cT [G, B, H] (None where the
    case leaves them out), w_hh [G, 4H, H] with 8 nonzeros per row, keep [T, B] or None."""
    gen = torch.Generator().manual_seed(c.seed)
    G, T, B = c.G, c.T, c.B
    shape = (G, T, B, H)
    sigm = (0.0, 0.25, 0.5, 0.75, 1.0) if c.sets == "rich" else (0.0, 0.5, 1.0)
    sym = (0.0, 0.5, -0.5, 1.0, -1.0)
    d = {"gi": _choice(gen, sigm, shape), "gf": _choice(gen, (0.0, 0.5, 1.0), shape), "gg": _choice(gen, sym, shape),
         "go": _choice(gen, sigm, shape), "cin": torch.randint(-2, 3, shape, generator=gen).double(), "tc": _choice(gen, sym, shape)}
    d["d_out"] = torch.randint(-3, 4, shape, generator=gen).double()
    d["d_hT"] = torch.randint(-2, 3, (G, B, H), generator=gen).double()
    d["d_cT"] = torch.randint(-2, 3, (G, B, H), generator=gen).double()
    w = torch.zeros(G, 4 * H, H, dtype=torch.float64)
    cols = torch.rand(G, 4 * H, H, generator=gen).argsort(-1)[..., :8]
    w.scatter_(2, cols, _choice(gen, (0.5, -0.5, 1.0, -1.0, 2.0, -2.0), (G, 4 * H, 8)))
    d["w_hh"] = w
    d["keep"] = _keep_mask(c.keep, T, B, gen)
    if not c.d_out:
        d["d_out"] = None
    if not c.d_last:
        d["d_hT"] = d["d_cT"] = None
    return d


def saved_of(d) -> Tuple[torch.Tensor, torch.Tensor]:
    """The fabricated values in the shape of ``pack_saved``: gates [T, G, B, 4, H], cells [T, G, B, 2, H]."""
    gates = torch.stack([d["gi"], d["gf"], d["gg"], d["go"]], 3).transpose(0, 1).contiguous()
    cells = torch.stack([d["cin"], d["tc"]], 3).transpose(0, 1).contiguous()
    return gates, cells


def backward_reference(d, want_state: bool = True, rounding: bool = True, defect: Optional[str] = None,
                       track: Optional[Dict[str, int]] = None, stats: Optional[Dict[str, float]] = None) -> Dict[str, Optional[torch.Tensor]]:
    """fp64 evaluation of lstm_seq_bwd_kernel's expressions in source order.  di, df, dg, d_o are rounded to bf16 (nearest even)
    before they enter d_xproj, the bias sums and the W_hh^T product; dh is multiplied by kt = keep[t] and dc by gf kt; d_h0 and d_c0
    are rounded once at the end.  Returns d_xproj [G, T, B, 4H], d_h0, d_c0 [G, B, H] (None when not wanted) and part [G, blocks,
    4H], all fp64.  ``track``: filled with the largest significant-bit count per kind of intermediate; ``stats``: coverage counts.
    ``defect``: one of BWD_DEFECTS, the emulation of a wrong kernel."""
    assert defect in (None,) + BWD_DEFECTS
    G, T, B, _ = d["gi"].shape
    nar = (lambda x: x) if not rounding else (lambda x: narrow(x, trunc=defect == "truncating_narrow"))
    keep, w = d["keep"], d["w_hh"]
    zeros = torch.zeros(G, B, H, dtype=torch.float64)

    def note(name, *xs):
        if track is not None:
            track[name] = max(track.get(name, 0), *(sig_bits(x) for x in xs))

    def count(name, hit, of):
        if stats is not None:
            stats[name] = stats.get(name, 0.0) + float(hit)
            stats[name + " of"] = stats.get(name + " of", 0.0) + float(of)

    dh = d["d_hT"] if d["d_hT"] is not None else zeros
    dc = d["d_cT"] if d["d_cT"] is not None and defect != "d_c_last_ignored" else zeros
    dx = [None] * T
    run = torch.zeros(G, B, 4 * H, dtype=torch.float64)           # a lane's running sums over the steps (dbs)
    for t in range(T - 1, -1, -1):
        tk = t + 1 if defect == "keep_of_next_tick" else t
        kt = keep[tk].view(1, B, 1) if keep is not None and tk < T else torch.ones(1, B, 1, dtype=torch.float64)
        to = t + 1 if defect == "d_out_of_next_tick" else t
        do = d["d_out"][:, to] if d["d_out"] is not None and to < T else zeros
        gi, gf, gg, go, cin, tc = (d[n][:, t] for n in ("gi", "gf", "gg", "go", "cin", "tc"))
        if defect == "f_g_tiles_swapped":
            gf, gg = gg, gf
        if defect == "df_from_cell_out":
            cin = gf * cin + gi * gg
        dd = dh + do
        a1 = dd * go; a2 = 1.0 - tc * tc; a3 = a1 * a2; dct = a3 + dc
        o1 = dd * tc; o2 = o1 * go; d_o = o2 * (1.0 - go)
        i1 = dct * gg; i2 = i1 * gi; di = i2 * (1.0 - gi)
        f1 = dct * cin; f2 = f1 * gf; df = f2 * (1.0 - gf)
        g1 = dct * gi; dg = g1 * ((1.0 - gg) if defect == "one_minus_gg" else (1.0 - gg * gg))
        c1 = dct * gf
        if stats is not None and t < T - 1:
            recv = (keep[t + 1] == 1).view(1, B, 1).expand(G, B, H) if keep is not None else torch.ones(G, B, H, dtype=torch.bool)
            count("W_hh^T product nonzero where received", (dh[recv] != 0).sum(), recv.sum())
            count("dc carry nonzero where received", (dc[recv] != 0).sum(), recv.sum())
        dc = c1 * kt
        note("cell-gradient terms", dd, a1, a3, dct, c1, dc)
        note("gate-gradient terms", o1, o2, d_o, i1, i2, di, f1, f2, df, g1, dg)
        v = [nar(di), nar(df), nar(dg), nar(d_o)]
        for name, raw, r in zip(("di", "df", "dg", "d_o"), (di, df, dg, d_o), v):
            count(name + " nonzero", (r != 0).sum(), r.numel())
            count("narrow() lossy", (r != raw).sum(), r.numel())
        dx[t] = torch.cat(v, -1)
        run = run + dx[t]
        note("running bias sums of a lane", run)
        if t > 0 or want_state or defect == "garbage_state_grads":
            if track is not None:   # rows with kt = 0 discard the product: whatever it rounds to, times 0
                track["W_hh^T product, any partial sum (bound)"] = max(track.get("W_hh^T product, any partial sum (bound)", 0), sum_bits_bound(dx[t] * kt, w))
            acc = torch.bmm(dx[t], w)
            note("W_hh^T product", acc * kt)
            dh = acc if defect == "kt_on_dc_only" else acc * kt
    d_x = torch.stack(dx, 1)
    nb = blocks(B)
    padded = torch.zeros(G, T, nb * BM, 4 * H, dtype=torch.float64)
    padded[:, :, :B] = d_x
    rows = padded.view(G, T, nb, BM, 4 * H)
    if track is not None:   # the kernel's own order: a lane's running sum over the steps (above), then the tree over the 16 rows
        v = rows.sum(1)
        for off in (8, 4, 2, 1):
            v = v[:, :, :off] + v[:, :, off:2 * off]
            note("part_dbias, the tree over a block's rows", v)
    if defect == "row15_not_in_part":
        rows = rows[:, :, :, :BM - 1]
    part = rows.sum((1, 3))
    if defect == "part_without_row_ok" and B % BM:
        part[:, -1] = float("nan")            # the padding lanes hold NaN
    note("part_dbias", part)
    out = {"d_xproj": d_x, "d_h0": nar(dh) if want_state else None, "d_c0": nar(dc) if want_state else None, "part": part}
    if defect == "garbage_state_grads" and not want_state:
        out["d_h0"], out["d_c0"] = nar(dh), nar(dc)       # buffers that must not exist, written
    return out


def backward_coverage(c: BwdCase, d, stats: Dict[str, float]) -> Dict[str, Tuple[float, float]]:
    """name -> (share or count, least allowed), from the ``stats`` of a reference run."""
    share = lambda n: stats.get(n, 0.0) / max(stats.get(n + " of", 0.0), 1.0)   # noqa: E731
    cov = {f"{n} nonzero": (share(f"{n} nonzero"), 0.08) for n in ("di", "df", "dg", "d_o")}
    if c.T >= 2:        # a single step's products of these sets have at most 8 significant bits: only a chain gives narrow() work
        cov["narrow() lossy"] = (share("narrow() lossy"), 0.01)
    keep = d["keep"]
    links = torch.ones(max(c.T - 1, 0), c.B) if keep is None else keep[1:]          # links[t] = 1: step t receives from step t + 1
    if c.T >= 2:
        cov["chains of two steps ending at even t"] = (float(links[0::2].sum()), 1)
        cov["W_hh^T product nonzero where received"] = (share("W_hh^T product nonzero where received"), 0.2)
        cov["dc carry nonzero where received"] = (share("dc carry nonzero where received"), 0.2)
    if c.T >= 3:
        cov["chains of two steps ending at odd t"] = (float(links[1::2].sum()), 1)
    return cov


def consistent_backward_data(G: int, T: int, B: int, seed: int, with_keep: bool) -> Tuple[Dict, Dict]:
    """Free fp64 data and the saved values an UNROUNDED forward pass over them leaves: what ties ``backward_reference`` to
    autograd through ``learner_exact.lstm_reference``.  Returns (forward data, backward data)."""
    gen = torch.Generator().manual_seed(seed)
    f = {"xproj": torch.randn(G, T, B, 4 * H, generator=gen, dtype=torch.float64), "w_hh": 0.15 * torch.randn(G, 4 * H, H, generator=gen, dtype=torch.float64),
         "h0": 0.5 * torch.randn(G, B, H, generator=gen, dtype=torch.float64), "c0": torch.randn(G, B, H, generator=gen, dtype=torch.float64),
         "bias": 0.3 * torch.randn(G, 4 * H, generator=gen, dtype=torch.float64), "bias2": 0.3 * torch.randn(G, 4 * H, generator=gen, dtype=torch.float64),
         "keep": (torch.rand(T, B, generator=gen) > 0.3).double() if with_keep else None}
    ref = forward_reference(f, rounding=False)
    gates, cells = ref["gates"].transpose(0, 1), ref["cells"].transpose(0, 1)            # [G, T, B, 4 | 2, H]
    b = {"gi": gates[:, :, :, 0], "gf": gates[:, :, :, 1], "gg": gates[:, :, :, 2], "go": gates[:, :, :, 3], "cin": cells[:, :, :, 0],
         "tc": cells[:, :, :, 1], "w_hh": f["w_hh"], "keep": f["keep"], "d_out": torch.randn(G, T, B, H, generator=gen, dtype=torch.float64),
         "d_hT": torch.randn(G, B, H, generator=gen, dtype=torch.float64), "d_cT": torch.randn(G, B, H, generator=gen, dtype=torch.float64)}
    return f, b
