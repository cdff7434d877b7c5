"""Exact known-answer data for the fused act tick (csrc/cat_act.hip): the cases, the parameter and observation generators, the
layer-rounded fp64 reference, the premises the exactness rests on, the coverage conditions and the comparison rule.  Used by
tests/act_exact_steps.py (on the GPU) and tests/test_act_exact_host.py (premises, coverage and the teeth, on the CPU).

Integer data alone cannot pin this chain, it has a tanh layer and an LSTM cell; it can once those saturate:
 - observations take three values per channel which the two scales turn into {0, 1, 2}; the scales differ, so swapping them shows;
 - conv1 / conv2 have weights and biases in {-1, 0, 1}: every sum is a small integer, the bf16 images hold it or round it once;
 - the 256-wide tanh layer has sparse weights in {0, +-16} and biases +-8: every pre-activation is 16 k + 8, |pre| >= 8, and tanh
   stored as bf16 is exactly +-1 (|tanh x| is within 2.3e-7 of 1 there, the rounding takes 2^-9);
 - W_ih rows hold three +-64, W_hh rows one +-128, the biases lie in {-2 .. 2}: every gate pre-activation has |pre| >= 24, the
   sigmoids are within e^-24 of 0 or 1, c stays an integer and h is 0 or bf16(tanh k), far from a rounding boundary;
 - the heads have sparse weights in {-1, 0, 1} and integer biases: all operands are multiples of 2^-8, every fp32 sum is exact in
   any order, so every layer's bf16 output is the exact value rounded once.
The reference is plain fp64 torch that rounds to bf16 (nearest even) where include/cat_act.h says the kernel does: c1, x2, f, h', c'
(also the state of the next tick), head layers 1 and 2, the logits.  Saturated gates leave residues below e^-24 max|c| where the
ideal value is 0; fast and fp64 transcendentals legitimately differ there, so the reference sets magnitudes below 2^-24 to 0 after
every rounding and ``act_equal`` asks bit equality wherever |want| >= 2^-24 and |got| <= 2^-24 where want is 0.

What rests on hardware behaviour nobody measured: __expf and rcp accurate to a few ulp at |x| >= 8 (the margins are 2^-9 against
2.3e-7 and 2^-3 bf16 ulp against 1e-6), and residues below 2^-24 (they are below 1e-11).  rcp(1.0) == 1.0 is not assumed (a gate
of 1 - a few ulp times an integer c rounds to that integer in bf16), nor is rcp(2.0) == 0.5: the tanh layer never sees 0, and no
nonzero value of the answer passes through tanh_fast(0).  Where c is ideally 0, h = go tanh_fast(residue) is ideally 0 as well and
falls under the 2^-24 rule: 1 - 2 rcp(2.0) of 0 or of 2^-24 (rcp one ulp low) passes, a larger one would fail the rule loudly in h
(about a quarter of its elements, which ``report`` of tests/act_exact_steps.py lists with their values), never pass a wrong kernel.

With every gate high in half of the elements h = go tanh(c) is nonzero in about a quarter, short of the 40 % the coverage asks, so
the data lean: 62 % of the flatten layer's weights (its inputs are >= 0) and all of W_ih's weights in the blocks i, f, o are positive.

Figures of the cases (python -m pytest tests/test_act_exact_host.py -s prints them per case), smallest .. largest over the cases:
  min |tanh-layer pre| 8.0; min |gate pre| 29.5; max c1 9 .. 12; max x2 60 .. 98 (so both are held exactly);
  partial-sum bounds over the grid: conv1 16 .. 21, conv2 171 .. 220, flatten 2376 .. 3944, lstm 82944, head 1 1937 .. 2267,
  head 2 4520 .. 6538, logits 8446 .. 11228 (limit 2^22); min distance of go tanh(c) from a bf16 rounding boundary 0.234 ulp (limit 0.125);
  coverage, all cases (N = 1 included): W_hh flips 12.3 .. 14.4 % of the gate signs; high: i 61.7 .. 69.5 %, f 65.1 .. 70.1 %,
  g 47.8 .. 51.7 %, o 64.0 .. 69.2 %; f positive 61.0 .. 65.3 %; h nonzero 44.9 .. 49.7 %; max |c| 5 (N = 1) .. 8 (N >= 33); all four
  greedy actions in every case; rows with tied maxima 0 .. 0.51 % (0 at N = 1), none of them tied at 0;
  keep, N >= 33: keep = 0 on 20.6 .. 21.2 % of the rows of every tick after the first;
  keep, N = 1 (the one condition replaced there, a share of one row cannot be 15 % in every tick and leave a state): of the 7 ticks
  after the first keep = 0 meets a nonzero h and c in 1 and keep = 1 in 6 (each asked in at least 1);
  88 .. 94 (N = 1), 1101 .. 1486 (N >= 33) distinct logit values; the reference has 0 at 50 .. 55 % of h, 27 .. 34 % of c, 0 .. 1.8 % of the logits."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from tests import learner_exact as lx

HID = 128
ZERO_TOL = 2.0 ** -24
DISTANCE_SCALE, TYPE_SCALE = 0.5, 0.25            # distances {0, 2, 4} and types {0, 4, 8} both become {0, 1, 2}
DISTANCES, TYPES = (0.0, 2.0, 4.0), (0, 4, 8)
BAND = 4096                                       # guard band of the parameter buffer, elements (8 KB: pointers keep 16-byte alignment)
NAMES = ("features_extractor.0.weight", "features_extractor.0.bias", "features_extractor.2.weight", "features_extractor.2.bias",
         "features_extractor.5.weight", "features_extractor.5.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0",
         "lstm.bias_hh_l0", "policy_head.0.weight", "policy_head.0.bias", "policy_head.2.weight", "policy_head.2.bias",
         "policy_head.4.weight", "policy_head.4.bias")          # _learn_native.ACT_PARAM_NAMES (the host test compares them)
FC_POS = 0.62                                     # share of +16 among the flatten layer's weights (its inputs are >= 0)
GATE_POS = (1.0, 1.0, 0.5, 1.0)                   # share of +64 in W_ih's blocks i, f, g, o
MUTANTS = ("conv1_taps", "conv2_halves", "flatten_order", "k_slice", "gates_i_f", "keep_h_only", "w_hh_transposed", "logit_rows",
           "other_network", "truncation")


@dataclass(frozen=True)
class ActCase:
    """T ticks of G networks (``sets`` parameter sets in the league form) over N envs with A agents each; network g reads env agent
    ``agents[g]``.  form: "plain" (cat_act_step), "league" (cat_act_league_step) or "collect" (cat_act_collect_step)."""
    G: int
    N: int
    A: int
    R: int
    row_tile: int
    T: int
    agents: Tuple[int, ...]
    form: str = "plain"
    first_agent_state: bool = False

    @property
    def sets(self) -> int:
        return 3 if self.form == "league" else self.G

    @property
    def seed(self) -> int:
        """Of the data: cases that differ in the row tile alone share their data and their reference."""
        return 1000 * self.R + 10 * self.N + {"plain": 0, "league": 1, "collect": 2}[self.form] + (5 if self.first_agent_state else 0)

    @property
    def id(self) -> str:
        return f"{self.form}-R{self.R}-N{self.N}-tile{self.row_tile}" + ("-first" if self.first_agent_state else "")


AGENTS = (2, 0, 3)                                # of A = 4; with N_COPS = 2 a thief comes first
N_COPS = 2
SEG_START = (0, 5, 38, 97)                        # the league form: no boundary on a tile edge
SEG_SET = ((0, 1, -1), (-1, 2, 0), (1, -1, 2))    # [g][segment]: a different set per (g, segment), one random segment per policy


def plain_cases():
    return [ActCase(3, N, 4, R, tile, 8, AGENTS) for R in (64, 90) for tile in (32, 64) for N in (1, 33, 97)]


def league_cases():
    return [ActCase(3, 97, 4, R, tile, 8, AGENTS, "league") for R in (64, 90) for tile in (32, 64)]


def collect_cases():
    return [ActCase(3, 33, 4, R, 32, 8, AGENTS, "collect", first) for R in (64, 90) for first in (False, True)]


def all_cases():
    return plain_cases() + league_cases() + collect_cases()


def data_cases():
    """One case per distinct data set (the row tile does not enter the data)."""
    seen, out = set(), []
    for c in all_cases():
        if c.seed not in seen:
            seen.add(c.seed)
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- comparison
def flush(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x.abs() < ZERO_TOL, torch.zeros_like(x), x)


def rounded(x: torch.Tensor, trunc: bool = False) -> torch.Tensor:
    """fp64 -> bf16 -> fp64 with magnitudes below 2^-24 set to 0: one storage point of the kernel."""
    return flush((lx.trunc_bf16(x) if trunc else lx.rne_bf16(x)).double())


def act_equal(got: torch.Tensor, want: torch.Tensor) -> bool:
    """got (bf16, or fp64 holding bf16 values) against the reference want (fp64 holding flushed bf16 values): bitwise equal wherever
    |want| >= 2^-24, |got| <= 2^-24 where want is 0."""
    g = got.detach().cpu()
    g16 = g if g.dtype == torch.bfloat16 else g.to(torch.bfloat16)
    w16 = want.to(torch.bfloat16)
    if g16.shape != w16.shape or not bool(torch.equal(g16.double(), g.double())):
        return False
    zero = want == 0
    same = g16.view(torch.int16) == w16.view(torch.int16)
    return bool((same | zero).all()) and bool((g16.double().abs()[zero] <= ZERO_TOL).all())


def zero_share(want: torch.Tensor) -> float:
    return float((want == 0).double().mean())


# ---------------------------------------------------------------------------------------------- parameters
def param_shapes(R: int) -> Dict[str, Tuple[int, ...]]:
    kfc = 32 * ((((R - 5) // 2 + 1) - 5) // 3 + 1)
    return dict(zip(NAMES, ((64, 2, 5), (64,), (32, 64, 5), (32,), (256, kfc), (256,), (512, 256), (512, HID), (512,), (512,),
                            (HID, HID), (HID,), (64, HID), (64,), (4, 64), (4,))))


def _sparse(gen, shape, nnz: int, value: float, pos=0.5) -> torch.Tensor:
    """[..., rows, cols] with ``nnz`` entries of +-value per row at distinct columns; ``pos``: the share of +value (a number, or one per row)."""
    cols = torch.rand(shape, generator=gen, dtype=torch.float64).argsort(-1)[..., :nnz]
    sign = (torch.rand(cols.shape, generator=gen, dtype=torch.float64) < torch.as_tensor(pos, dtype=torch.float64).view(-1, 1)).double() * 2 - 1
    return torch.zeros(shape, dtype=torch.float64).scatter_(-1, cols, sign * value)


def make_params(sets: int, R: int, seed: int) -> Dict[str, torch.Tensor]:
    """name -> fp64 [sets, ...], every set drawn on its own (all values are bf16s)."""
    gen = torch.Generator().manual_seed(seed)
    shapes = param_shapes(R)

    def ints(name, lo, hi):                                       # integers lo .. hi
        return torch.randint(lo, hi + 1, (sets,) + shapes[name], generator=gen).double()

    def sparse(name, nnz, value, pos=0.5):                        # nnz entries of +-value per row
        return _sparse(gen, (sets,) + shapes[name], nnz, value, pos)

    def conv1_taps(name):                                         # {-1, 0, 1}, the positive taps sparse (1/6): lx.trunk_params
        u = torch.rand((sets,) + shapes[name], generator=gen, dtype=torch.float64)
        return (u < 1 / 6).double() - (u > 2 / 3).double()

    gate_pos = torch.tensor(GATE_POS).repeat_interleave(HID)      # per row of W_ih: the blocks i, f, g, o
    draw = {                                                      # drawn in this order from the one generator
        "features_extractor.0.weight": conv1_taps,
        "features_extractor.0.bias":   lambda n: ints(n, -1, 1),
        "features_extractor.2.weight": lambda n: ints(n, -1, 1),
        "features_extractor.2.bias":   lambda n: ints(n, -1, 1),
        "features_extractor.5.weight": lambda n: sparse(n, 6, 16.0, FC_POS),
        "features_extractor.5.bias":   lambda n: ints(n, 0, 1) * 16 - 8,
        "lstm.weight_ih_l0":           lambda n: sparse(n, 3, 64.0, gate_pos),
        "lstm.weight_hh_l0":           lambda n: sparse(n, 1, 128.0),
        "lstm.bias_ih_l0":             lambda n: ints(n, -2, 2),
        "lstm.bias_hh_l0":             lambda n: ints(n, -2, 2),
        "policy_head.0.weight":        lambda n: sparse(n, 8, 1.0),
        "policy_head.0.bias":          lambda n: ints(n, -1, 1),
        "policy_head.2.weight":        lambda n: sparse(n, 8, 1.0),
        "policy_head.2.bias":          lambda n: ints(n, -1, 1),
        "policy_head.4.weight":        lambda n: sparse(n, 8, 1.0),
        "policy_head.4.bias":          lambda n: ints(n, -2, 2),
    }
    assert tuple(draw) == NAMES
    P = {n: draw[n](n) for n in NAMES}
    assert all(P[n].shape[1:] == shapes[n] and torch.equal(lx.rne_bf16(P[n]).double(), P[n]) for n in NAMES)
    return P


def param_layout(R: int) -> Tuple[Dict[str, int], int]:
    """(offset of every block inside one network's parameters, the stride between networks): elements, multiples of 8."""
    off, at = {}, 0
    for n, shp in param_shapes(R).items():
        off[n] = at
        at += -(-int(torch.Size(shp).numel()) // 8) * 8
    return off, at + 8                              # one spare 16 bytes between the networks


def flat_params(P: Dict[str, torch.Tensor], R: int) -> torch.Tensor:
    """The bf16 buffer [BAND | set 0 | set 1 | ... | BAND]; the bands and the padding hold NaN."""
    off, stride = param_layout(R)
    sets = P[NAMES[0]].shape[0]
    flat = torch.full((2 * BAND + sets * stride,), float("nan"), dtype=torch.bfloat16)
    for n in NAMES:
        for k in range(sets):
            at = BAND + k * stride + off[n]
            flat[at:at + P[n][k].numel()] = P[n][k].flatten().to(torch.bfloat16)
    return flat


def param_views(flat: torch.Tensor, R: int) -> Dict[str, torch.Tensor]:
    """name -> bf16 [sets, ...] view into ``flat`` (on any device): what ``_learn_native.act_params`` takes."""
    off, stride = param_layout(R)
    sets = (flat.numel() - 2 * BAND) // stride
    out = {}
    for n, shp in param_shapes(R).items():
        inner, st = [], 1
        for d in reversed(shp):
            inner.insert(0, st)
            st *= d
        out[n] = flat.as_strided((sets,) + shp, [stride] + inner, BAND + off[n])
    return out


# ---------------------------------------------------------------------------------------------- observations, keep, uniforms
def make_inputs(c: ActCase) -> Dict[str, torch.Tensor]:
    """obs_distance f16 / obs_type u8 [T, N, A, R], shared_distance / shared_type [T, N, 2, R] drawn the same way, keep fp32 [T, N]
    (tick 0: all 1; later 0 on a fifth of the rows, at least one, or with probability 1/4 where there is one row), uniform fp32
    [T, G, N], and the state before the first tick (zero; the league form's random rows hold sentinels that must survive)."""
    gen = torch.Generator().manual_seed(c.seed)
    pick = lambda vals, shape, dt: torch.tensor(vals, dtype=dt)[torch.randint(0, 3, shape, generator=gen)]
    d = {"obs_distance": pick(DISTANCES, (c.T, c.N, c.A, c.R), torch.float16), "obs_type": pick(TYPES, (c.T, c.N, c.A, c.R), torch.uint8),
         "shared_distance": pick(DISTANCES, (c.T, c.N, 2, c.R), torch.float16), "shared_type": pick(TYPES, (c.T, c.N, 2, c.R), torch.uint8)}
    keep = torch.ones(c.T, c.N)
    for t in range(1, c.T):
        if c.N == 1:
            keep[t, 0] = float(torch.rand((), generator=gen) >= 0.25)
        else:
            keep[t, torch.randperm(c.N, generator=gen)[:-(-c.N // 5)]] = 0.0
    d["keep"] = keep
    d["uniform"] = torch.rand(c.T, c.G, c.N, generator=gen)
    h0, c0 = torch.zeros(c.G, c.N, HID, dtype=torch.float64), torch.zeros(c.G, c.N, HID, dtype=torch.float64)
    if c.form == "league":
        for g in range(c.G):
            for s, k in enumerate(SEG_SET[g]):
                if k < 0:
                    h0[g, SEG_START[s]:SEG_START[s + 1]] = 0.5
                    c0[g, SEG_START[s]:SEG_START[s + 1]] = 3.0
    d["h0"], d["c0"] = h0, c0
    return d


def scaled(dist: torch.Tensor, typ: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernel's conversion: fp32 value x scale rounded to bf16, as fp64."""
    return ((dist.float() * DISTANCE_SCALE).to(torch.bfloat16).double(), (typ.float() * TYPE_SCALE).to(torch.bfloat16).double())


def policy_rows(c: ActCase, d, t: int) -> torch.Tensor:
    """[G, N, 2R] fp64: [distance | type] of agent agents[g]."""
    dist, typ = scaled(d["obs_distance"][t], d["obs_type"][t])
    return torch.stack([torch.cat([dist[:, a], typ[:, a]], -1) for a in c.agents])


def value_rows(c: ActCase, d, t: int) -> torch.Tensor:
    """[G, N, 4R] fp64: [shared distance | shared type | distance | type] of the state agent (agent 0 or agents[g]) and its team."""
    dist, typ = scaled(d["obs_distance"][t], d["obs_type"][t])
    sd, st = scaled(d["shared_distance"][t], d["shared_type"][t])
    rows = []
    for a in c.agents:
        si = 0 if c.first_agent_state else a
        team = 0 if si < N_COPS else 1
        rows.append(torch.cat([sd[:, team], st[:, team], dist[:, si], typ[:, si]], -1))
    return torch.stack(rows)


# ---------------------------------------------------------------------------------------------- the reference
def tick_one(P: Dict[str, torch.Tensor], x, h, cc, keep, R: int, mut: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """One network (P: name -> fp64 block) on rows x [n, 2R] with state h, cc [n, 128] and keep [n]: fp64, rounded to bf16 and flushed
    at the kernel's storage points.  ``mut``: one of MUTANTS, a defect in the index arithmetic (the host test's teeth)."""
    F = torch.nn.functional
    n = x.shape[0]
    trunc = mut == "truncation"
    w1, w2, wfc, whh = P[NAMES[0]], P[NAMES[2]], P[NAMES[4]], P[NAMES[7]]
    if mut == "conv1_taps":
        w1 = w1[:, :, [0, 3, 2, 1, 4]]
    if mut == "conv2_halves":
        w2 = torch.cat([w2[:, 32:], w2[:, :32]], 1)
    if mut == "k_slice":                                         # the last 32 columns: slice 13 at R = 90, 9 at R = 64
        wfc = torch.cat([wfc[:, :-32], torch.zeros_like(wfc[:, -32:])], 1)
    if mut == "w_hh_transposed":
        whh = whh.reshape(HID, 4 * HID).t()
    c1 = rounded(torch.relu(F.conv1d(x.view(n, 2, R), w1, P[NAMES[1]], stride=2)))
    x2 = rounded(torch.relu(F.conv1d(c1, w2, P[NAMES[3]], stride=3)))                   # [n, 32, L2]
    flat = (x2.transpose(1, 2) if mut == "flatten_order" else x2).reshape(n, -1)       # (channel, position)
    pre_fc = flat @ wfc.t() + P[NAMES[5]]
    f = rounded(torch.tanh(pre_fc))
    hp, cp = h * keep.view(n, 1), cc if mut == "keep_h_only" else cc * keep.view(n, 1)
    bias = P[NAMES[8]] + P[NAMES[9]]
    pre_in = f @ P[NAMES[6]].t() + bias
    pre = pre_in + hp @ whh.t()
    gi, gf, gg, go = pre.chunk(4, dim=-1)
    if mut == "gates_i_f":
        gi, gf = gf, gi
    c_raw = torch.sigmoid(gf) * cp + torch.sigmoid(gi) * torch.tanh(gg)
    h_raw = torch.sigmoid(go) * torch.tanh(c_raw)
    hn, cn = rounded(h_raw), rounded(c_raw)
    y1 = rounded(torch.relu(hn @ P[NAMES[10]].t() + P[NAMES[11]]), trunc)
    y2 = rounded(torch.relu(y1 @ P[NAMES[12]].t() + P[NAMES[13]]), trunc)
    z = rounded(y2 @ P[NAMES[14]].t() + P[NAMES[15]], trunc)
    if mut == "logit_rows":
        z = z[:, [0, 2, 1, 3]]
    return {"logits": z, "h": hn, "c": cn, "x": x, "c1": c1, "x2": flat, "pre_fc": pre_fc, "f": f, "hp": hp, "pre_in": pre_in, "pre": pre,
            "h_raw": h_raw, "y1": y1, "y2": y2}


def network_of(c: ActCase, g: int, n0: int) -> int:
    """The parameter set that plays row n0 of policy g (-1: uniformly random)."""
    if c.form != "league":
        return g
    s = max(i for i, b in enumerate(SEG_START[:-1]) if b <= n0)
    return SEG_SET[g][s]


def row_blocks(c: ActCase):
    return list(zip(SEG_START[:-1], SEG_START[1:])) if c.form == "league" else [(0, c.N)]


def reference(c: ActCase, P, d, mut: Optional[str] = None, keep_one: bool = False, details: bool = False):
    """The T ticks: a list of {"logits" [G, N, 4], "h", "c" [G, N, 128], "net" [G, N] (bool: a network played the row)} per tick, and
    with ``details`` the per-block intermediates of tick_one as well.  ``keep_one``: keep = 1 throughout (the kernel's keep = NULL)."""
    h, cc = d["h0"].clone(), d["c0"].clone()
    out = []
    for t in range(c.T):
        x = policy_rows(c, d, t)
        keep = torch.ones(c.N, dtype=torch.float64) if keep_one else d["keep"][t].double()
        z = torch.zeros(c.G, c.N, 4, dtype=torch.float64)
        net = torch.zeros(c.G, c.N, dtype=torch.bool)
        hn, cn, blocks = h.clone(), cc.clone(), []
        for g in range(c.G):
            for a, b in row_blocks(c):
                k = network_of(c, g, a)
                if k < 0:
                    continue
                if mut == "other_network":
                    k = (k + 1) % c.sets
                r = tick_one({n_: P[n_][k] for n_ in NAMES}, x[g, a:b], h[g, a:b], cc[g, a:b], keep[a:b], c.R, mut)
                z[g, a:b], hn[g, a:b], cn[g, a:b], net[g, a:b] = r["logits"], r["h"], r["c"], True
                blocks.append(r)
        h, cc = hn, cn
        out.append({"logits": z, "h": h, "c": cc, "net": net, **({"blocks": blocks} if details else {})})
    return out


def first_max(z: torch.Tensor) -> torch.Tensor:
    """The lowest index of the largest logit (argmax does not promise which on ties)."""
    return (z == z.amax(-1, keepdim=True)).int().cumsum(-1).eq(0).sum(-1)


def random_action(u: torch.Tensor) -> torch.Tensor:
    """min(3, int(4 u)) in fp32, the kernel's rule for a random policy."""
    return (4.0 * u.float()).to(torch.int32).clamp(max=3)


# ---------------------------------------------------------------------------------------------- premises and coverage
def _boundary_distance(v: torch.Tensor) -> float:
    """Smallest distance, in bf16 ulps, of the magnitudes >= 2^-24 in v from a bf16 rounding boundary (a half-way point)."""
    a = v.abs().flatten()
    a = a[a >= ZERO_TOL]
    if a.numel() == 0:
        return 0.5
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    frac = torch.remainder(a / ulp, 1.0)
    return float((frac - 0.5).abs().min())


def premises(c: ActCase, P=None, d=None, ref=None) -> Dict[str, Tuple[float, float]]:
    """name -> (value, limit) from the reference's own intermediates: names that begin with "min" need value >= limit, the others
    value <= limit (``premise_holds``)."""
    P = P if P is not None else make_params(c.sets, c.R, c.seed)
    d = d if d is not None else make_inputs(c)
    ref = ref if ref is not None else reference(c, P, d, details=True)
    blocks = [(b, k) for tick in ref for b, k in zip(tick["blocks"], _block_sets(c))]
    grid = 2.0 ** -8

    def bound(wname, key, k, b, g_):                              # max over outputs of sum_k |w| |x|, over the grid
        return float((b[key].abs() @ P[wname][k].abs().flatten(1).t()).max()) / g_

    def conv_bound(wname, key, b, k, stride):
        x = b[key] if key != "x" else b[key].view(-1, 2, c.R)
        return float(torch.nn.functional.conv1d(x.abs(), P[wname][k].abs(), stride=stride).max())

    out = {
        "min |tanh-layer pre-activation|": (min(float(b["pre_fc"].abs().min()) for b, _ in blocks), 8.0),
        "min |gate pre-activation|": (min(float(b["pre"].abs().min()) for b, _ in blocks), 24.0),
        "max c1": (max(float(b["c1"].max()) for b, _ in blocks), float(lx.BF16_INT)),
        "min distance of go tanh(c) from a bf16 rounding boundary (ulp)": (min(_boundary_distance(b["h_raw"]) for b, _ in blocks), 2.0 ** -3),
        "partial sums conv1": (max(conv_bound(NAMES[0], "x", b, k, 2) + 1 for b, k in blocks), lx.SUM_LIMIT),
        "partial sums conv2": (max(conv_bound(NAMES[2], "c1", b, k, 3) + 1 for b, k in blocks), lx.SUM_LIMIT),
        "partial sums flatten layer": (max(bound(NAMES[4], "x2", k, b, 1.0) + 8 for b, k in blocks), lx.SUM_LIMIT),
        "partial sums lstm / 2^-8": (max(float((b["f"].abs() @ P[NAMES[6]][k].abs().t() + b["hp"].abs() @ P[NAMES[7]][k].abs().t()).max()) + 4
                                         for b, k in blocks) / grid, lx.SUM_LIMIT),
        "partial sums head 1 / 2^-8": (max(bound(NAMES[10], "h", k, b, grid) + 1 / grid for b, k in blocks), lx.SUM_LIMIT),
        "partial sums head 2 / 2^-8": (max(bound(NAMES[12], "y1", k, b, grid) + 1 / grid for b, k in blocks), lx.SUM_LIMIT),
        "partial sums logits / 2^-8": (max(bound(NAMES[14], "y2", k, b, grid) + 2 / grid for b, k in blocks), lx.SUM_LIMIT),
    }
    out["heads on the 2^-8 grid (max off-grid part)"] = (max(float(torch.remainder(b[key] / grid, 1.0).max())
                                                             for b, _ in blocks for key in ("h", "y1", "y2", "logits")), 0.0)
    return out


def premise_holds(name: str, value: float, limit: float) -> bool:
    return value >= limit if name.startswith("min") else value <= limit


def _block_sets(c: ActCase):
    """The parameter set of every block of one tick's ``blocks``, in reference()'s order."""
    return [network_of(c, g, a) for g in range(c.G) for a, _ in row_blocks(c) if network_of(c, g, a) >= 0]


def coverage(c: ActCase, P=None, d=None, ref=None) -> Dict[str, Tuple[float, float, float]]:
    """name -> (value, lowest, highest allowed): what makes the data able to see a defect, from the reference alone."""
    P = P if P is not None else make_params(c.sets, c.R, c.seed)
    d = d if d is not None else make_inputs(c)
    ref = ref if ref is not None else reference(c, P, d, details=True)
    cat = lambda key, ticks: torch.cat([b[key].flatten() for t in ticks for b in ref[t]["blocks"]])
    later, every = range(1, c.T), range(c.T)
    pre, pre_in = cat("pre", later), cat("pre_in", later)
    out = {"W_hh flips the gate's sign (ticks after the first)": (float(((pre > 0) != (pre_in > 0)).double().mean()), 0.03, 1.0)}
    for j, name in enumerate("ifgo"):
        gate = torch.cat([b["pre"].chunk(4, -1)[j].flatten() for t in every for b in ref[t]["blocks"]])
        out[f"gate {name} high"] = (float((gate > 0).double().mean()), 0.25, 0.75)
    net = torch.stack([t["net"] for t in ref])
    z = torch.stack([t["logits"] for t in ref])[net]
    top = z.amax(-1, keepdim=True)
    tied = (z == top).sum(-1) > 1
    out.update({
        "f positive": (float((cat("f", every) > 0).double().mean()), 0.30, 0.70),
        "h nonzero": (float((cat("h", every) != 0).double().mean()), 0.40, 1.0),
        "max |c|": (float(cat("c", every).abs().max()), 3.0, float(lx.BF16_INT)),
        "greedy actions that occur": (float(first_max(z).unique().numel()), 4.0, 4.0),
        "rows with tied maxima": (float(tied.double().mean()), 0.0, 0.01),
        "rows whose tied maximum is 0 (a residue could pick another)": (float((tied & (top[..., 0] == 0)).sum()), 0.0, 0.0),
    })
    if c.N > 1:
        out["least share of rows with keep = 0 in a tick after the first"] = (float((d["keep"][1:] == 0).float().mean(1).min()), 0.15, 1.0)
    else:               # one row cannot have keep = 0 in every tick and still carry a state: both must happen, each in some tick
        state = [t for t in later if bool((ref[t - 1]["h"] != 0).any()) and bool((ref[t - 1]["c"] != 0).any())]      # h and c come in nonzero
        out["ticks after the first with keep = 0 on a nonzero state (one row)"] = (float(sum(float(d["keep"][t, 0]) == 0 for t in state)), 1.0, c.T - 1.0)
        out["ticks after the first with keep = 1 on a nonzero state (one row)"] = (float(sum(float(d["keep"][t, 0]) == 1 for t in state)), 1.0, c.T - 1.0)
    return out


def figures(c: ActCase, P, d, ref) -> Dict[str, float]:
    """What the host test prints next to the premises: not conditions."""
    z = torch.stack([t["logits"] for t in ref])[torch.stack([t["net"] for t in ref])]
    blocks = [b for t in ref for b in t["blocks"]]
    return {"max x2": max(float(b["x2"].max()) for b in blocks), "distinct logit values": float(z.unique().numel()),
            "zero share h": zero_share(torch.cat([b["h"].flatten() for b in blocks])),
            "zero share c": zero_share(torch.cat([b["c"].flatten() for b in blocks])), "zero share logits": zero_share(z)}
