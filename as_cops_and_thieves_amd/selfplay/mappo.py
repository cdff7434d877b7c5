"""MAPPO on the batched env.

What the reference runs (``src/self_play_driver.py`` -> ``training/orchestration.py`` ->
``utils/agent_learning_utils.py:172-230`` -> skrl ``MAPPO`` + ``SequentialTrainer``) and what this module
restates, on the device env:

* every agent owns a policy and a value network and is optimised independently (skrl MAPPO); here the agents of
  one ROLE share one stacked network evaluation (``stacked.py``) -- same per-agent parameters, one launch;
* per-role hyper-parameters ``CFG_AGENT`` / ``CFG_AGENT_COP`` / ``CFG_AGENT_THIEF``
  (``src/configs/mappo_config.py:5-50``; the driver passes ``CFG_AGENT`` for both roles, which is the default);
* the timestep-driven schedule of one ``trainer.train()`` call: ``random_timesteps`` uniformly random actions,
  no update before ``learning_starts`` (``mappo_config.py:9-10``), all policies frozen until
  ``policy_freeze_duration`` and the value networks released at ``opponent_freeze_duration`` (``CFG_TRAINER``,
  ``mappo_config.py:52-63``; the reference implements the two durations by a local patch to skrl's trainers,
  ``README.md:58-154``).  A timestep is one tick of the env batch, as in the reference's single-env loop;
* PPO as skrl writes it [SKRL-RECALL: skrl is not installed here]: GAE(0.99, 0.95) with per-agent advantage
  normalisation, clipped surrogate, entropy bonus, scaled MSE value loss, one joint gradient-norm clip over the
  agent's policy + value parameters, Adam, and the per-minibatch KL early stop ("break": the rest of the epoch's
  minibatches of THAT agent are skipped, the next epoch runs again).

MI355X shape of the update: one flat fp32 master buffer per role, bf16 compute copy, gradients accumulate into one
flat buffer, ONE all-reduce per optimiser step (gradients and the KL statistics in the same buffer, so every rank
takes the same early-stop decision), per-agent clip and a masked Adam as a few flat kernels, KL / freeze decisions
as device-side gates -- no host synchronisation inside an update, so the minibatch step is captured in HIP graphs.
"""
from __future__ import annotations

import dataclasses
import math
import warnings
from typing import Sequence, Dict, List, Optional, Tuple

import torch

from .. import packing
from .. import _learn_native
from .models import state_width
from .stacked import (FlatParams, StackedNet, adam_state_dict, agent_state_dict, init_from_modules, load_adam_state_dict,
                      load_agent_state_dict,
                      role_param_shapes)


@dataclasses.dataclass
class RoleConfig:
    """skrl MAPPO agent configuration of one role (``src/configs/mappo_config.py:5-50``)."""
    rollouts: int = 4096                   # mappo_config.py:8: ticks of the (single) env per update.  The trainer's rollout length is
                                           # ``TrainerConfig.horizon`` (default 128 ticks of thousands of envs); pass horizon=cfg.rollouts
                                           # for the reference's own setting (tests/test_gpu_mappo.py runs it at 32 envs)
    learning_epochs: int = 4
    mini_batches: int = 4
    discount_factor: float = 0.99          # skrl MAPPO_DEFAULT_CONFIG
    gae_lambda: float = 0.95               # skrl MAPPO_DEFAULT_CONFIG ("lambda")
    learning_rate: float = 1e-4
    ratio_clip: float = 0.15
    value_loss_scale: float = 0.5
    entropy_loss_scale: float = 0.02
    grad_norm_clip: float = 0.5
    kl_threshold: float = 0.015
    random_timesteps: int = 10_000
    learning_starts: int = 15_000
    # Schedules (build-side options; the reference trains at constant values).  All defaults mean "off": see ``scheduled``.
    lr_schedule: str = "constant"          # "constant", "linear" (learning_rate -> lr_final over schedule_updates updates) or
                                           # "kl_adaptive" (skrl's KLAdaptiveLR [SKRL-RECALL], per agent: after every epoch the rate is
                                           # divided by lr_factor where the epoch's mean minibatch KL is above lr_kl_target * lr_kl_factor,
                                           # multiplied where it is below lr_kl_target / lr_kl_factor, and kept inside [lr_min, lr_max])
    lr_final: Optional[float] = None       # end value for "linear"
    lr_kl_target: float = 0.008            # the next five: KLAdaptiveLR's defaults.  Not ``kl_threshold``, which stays the early-stop gate
    lr_kl_factor: float = 2.0
    lr_factor: float = 1.5
    lr_min: float = 1e-6
    lr_max: float = 1e-2
    entropy_final: Optional[float] = None      # linear anneal of entropy_loss_scale to this value
    ratio_clip_final: Optional[float] = None   # linear anneal of ratio_clip to this value
    schedule_updates: int = 0              # updates over which the linear anneals run: progress = min(1, finished updates / this)


LR_SCHEDULES = ("constant", "linear", "kl_adaptive")


def scheduled(cfg: RoleConfig) -> bool:
    """True when ``cfg`` asks for any schedule: its learner then keeps the three hyper-parameters in device memory (``RoleLearner.hyper``)."""
    return cfg.lr_schedule != "constant" or cfg.entropy_final is not None or cfg.ratio_clip_final is not None


def check_schedule(cfg: RoleConfig) -> None:
    """ValueError naming the field of a schedule configuration that cannot run."""
    if cfg.lr_schedule not in LR_SCHEDULES:
        raise ValueError(f"RoleConfig.lr_schedule must be one of {LR_SCHEDULES}, got {cfg.lr_schedule!r}")
    if cfg.lr_schedule == "linear" and cfg.lr_final is None:
        raise ValueError('RoleConfig.lr_final: lr_schedule="linear" needs the end value')
    linear = cfg.lr_schedule == "linear" or cfg.entropy_final is not None or cfg.ratio_clip_final is not None
    if linear and (isinstance(cfg.schedule_updates, bool) or not isinstance(cfg.schedule_updates, int) or cfg.schedule_updates <= 0):
        raise ValueError(f"RoleConfig.schedule_updates must be a positive number of updates for a linear schedule, got {cfg.schedule_updates!r}")
    if not cfg.lr_factor >= 1.0:            # the KL rule's numbers: what cat_ppo_schedule_step rejects, whatever the mode
        raise ValueError(f"RoleConfig.lr_factor must be >= 1, got {cfg.lr_factor!r}")
    if not cfg.lr_kl_factor >= 1.0:
        raise ValueError(f"RoleConfig.lr_kl_factor must be >= 1, got {cfg.lr_kl_factor!r}")
    if not cfg.lr_min <= cfg.lr_max:
        raise ValueError(f"RoleConfig.lr_min must be <= lr_max, got {cfg.lr_min!r} > {cfg.lr_max!r}")


CFG_AGENT = RoleConfig()                                                                       # mappo_config.py:41-50
CFG_AGENT_COP = RoleConfig()                                                                   # :19-28
CFG_AGENT_THIEF = RoleConfig(learning_epochs=3, mini_batches=8, entropy_loss_scale=0.01,      # :30-39
                             learning_rate=3e-4, ratio_clip=0.2)


@dataclasses.dataclass
class TrainerConfig:
    """``CFG_TRAINER`` (``mappo_config.py:52-63``) plus the build-side knobs."""
    timesteps: int = 100_000               # TrainingConfig.training_timesteps_per_role_training
    opponent_freeze_duration: int = 15_000
    policy_freeze_duration: int = 15_000
    horizon: int = 128                     # ticks per rollout; a multiple of ``bptt``.  With 16 (one BPTT window, the setting
                                           # of the bench line's first learner figure) the cops do not learn to catch even
                                           # random thieves in 262 M env-steps; with 128 they do (tests/test_gpu_mappo.py)
    bptt: int = 16                         # BPTT window (reference LSTM sequence_length).  A rollout of W = horizon / bptt
                                           # windows trains on W * num_envs sequences per update: the same number of
                                           # optimiser steps over W times the data (the update's cost is dominated by
                                           # its kernel COUNT, which does not grow with W)
    compute_bf16: bool = True              # bf16 compute copy of the weights on a GPU (fp32 master + fp32 Adam)
    check_device_errors: bool = True       # read the env core's device error word once per update (raises on any flag)
    graph_rollout: bool = True             # capture the T-tick rollout (env ticks + all networks) in one HIP graph
    graph_update: bool = True              # capture the minibatch step (forward, losses, backward / clip, Adam)
    reference_q11: bool = False            # True: every critic sees the alphabetically first agent's channels (quirk Q11)
    random_action_roles: Tuple[str, ...] = ()   # roles that act uniformly at random throughout (a fixed random opponent)
    deferred_values: bool = True           # kernel path: the critics do not run tick by tick (nothing in a rollout reads
                                           # their output) but once per BPTT window after the last tick, on all its ticks
    recurrent: bool = True                 # True: the LSTM pair the reference's drivers use (orchestration.py:52,121:
                                           # initialize_lstm_models_for_mappo).  False: its non-recurrent pair (policy_net.py:9-45,
                                           # value_net.py:8-34, model_utils.py:45-77 initialize_models_for_mappo): Policy = conv trunk +
                                           # MLP on the agent's own rays, Value = an MLP over the WHOLE flattened shared state of all
                                           # agents; stacked and trained by the same learner (torch packing path, the dense kernels)
    resident_random_phase: bool = True     # while EVERY learner is inside its random_timesteps and none is due an update, the env is
                                           # advanced by the resident rollout launch (VecCopsEnv.rollout_random: cat_rollout_fused,
                                           # uniformly random Philox actions) instead of tick by tick -- skrl neither evaluates a
                                           # network nor keeps a transition of that phase (no update before learning_starts, and the
                                           # rollout memory is overwritten by then), so only the env's state after it matters
    normalize_inputs: bool = False         # False = the reference: raw distances (0..400) and type codes (0..4) go into the
                                           # convolutions (skrl's state_preprocessor is None).  True (build-side option):
                                           # distances / ray length, types / 4 -- see tools/learn_curve.py
    episode_stats: bool = False            # with an env that offers ``episode_stats`` / ``episode_tracker`` (``VecCopsEnv(track_episodes=True)``): ``read_stats``
                                           # adds the episodes, the cops' win rate, the mean episode length and every agent's mean
                                           # return of the episodes finished during this ``train()`` call.  The accounting rides inside the
                                           # env's step (captured and replayed with the rollout graph); nothing of the rollout or the update
                                           # changes
    frame_skip: int = 1                    # env ticks per decision (action repeat): every step of the rollout is ``env.step(actions,
                                           # repeat=frame_skip)`` / ``step_raw(..., repeat=frame_skip)``, one resident launch that holds
                                           # the actions for up to that many ticks and stops a slot where its episode ends.  Above 1 a
                                           # "tick" of ``horizon``, ``bptt``, ``timesteps``, the freeze durations and the role configs'
                                           # ``random_timesteps`` / ``learning_starts`` is a DECISION, ``discount_factor`` and ``lambda``
                                           # apply per decision, and the rewards the learner sees are the env's fp32 window sums (the
                                           # trainer adds nothing up itself).  ``read_stats()["env_ticks"]`` counts the env ticks played.
                                           # The resident random-phase fast-forward stays as it is: it plays its span in env ticks,
                                           # one per counted timestep
    fused_collect: bool = False            # True: a policy-driven tick of a learner is ONE launch of ``cat_act_collect_step`` (include/cat_act.h) --
                                           # observation packing, the whole policy chain, the draw, and the stores of the packed rows, the
                                           # action, its log-probability and the window-start state into the rollout buffers -- instead of
                                           # cat_rollout_pack + the per-layer chain + cat_rollout_sample.  Needs a GPU, bf16 compute, the
                                           # recurrent pair, 64 or 90 rays, an env with ``raw_outputs`` / ``step_raw``, ``deferred_values`` and no
                                           # ``random_action_roles``: the trainer raises ValueError otherwise.  Random-phase ticks and roles
                                           # played by ``set_opponent`` actors stay on their own paths.  The kernel rounds where the chain does
                                           # but accumulates the LSTM gates unrounded (include/cat_act.h), so actions differ from the chain's in
                                           # the last bits of the logits: same distribution, not the same trajectory
    value_norm: bool = False               # True: running value normalisation (the MAPPO paper's first implementation recommendation; skrl's
                                           # ``value_preprocessor``, which the reference leaves off).  Every learner keeps per-agent running moments
                                           # (n, mean, M2) of the raw returns in f64 (``RoleLearner.vn_state``) and the scale (mu, sigma) they give
                                           # (``vn_scale``, (0, 1) at first).  The critic is trained on (return - mu) / (sigma + 1e-8) and its outputs
                                           # are normalised values: the GAE scan denormalises them as it reads them (``cat_ppo_gae_scan_scaled``),
                                           # the moments take in every update's raw returns (``cat_ppo_moments``: fixed order, bit-reproducible,
                                           # include/cat_ppo.h), then the targets are normalised with the new scale.  False: nothing is added
    geodesic_shaping: float = 0.0          # W > 0: geodesic potential-based reward shaping (Ng, Harada and Russell 1999; ``selfplay/shaping.py``).
                                           # Every learner's reward rows take ``F = gamma Phi(s') - Phi(s)`` with its own ``discount_factor`` and
                                           # ``Phi = -W min(hops, cap)`` for a cop, ``+shaping_scale_thief min(hops, cap)`` for a thief, hops the
                                           # shortest-path separation from the nearest opponent on the map's grid (``navigation.NavField``): one
                                           # launch of ``cat_render_nav_shape`` per learner and tick inside the captured rollout, and one at its top
                                           # that primes the separations from the env's current state.  ``F`` is kept in ``buf["shape"]``;
                                           # ``read_stats`` adds ``shaping/<agent>`` and ``geodesic_hops/<agent>``.  The env's own rewards, episode
                                           # statistics and observations are untouched.  Needs an env built with ``final_positions=True`` that offers
                                           # ``raw_outputs``.  0 (the reference trains unshaped): no shaper, no field, no buffer, no launch
    shaping_scale_thief: Optional[float] = None     # the thieves' scale; None: ``geodesic_shaping``.  0 leaves the thieves unshaped
    shaping_cap: int = 64                  # hop counts above it count as it (1 .. 65534): the potential is bounded by scale * cap
    spawn_curriculum: Optional[Tuple[int, int]] = None     # (lo, hi): a geodesic start-state curriculum (``selfplay/curriculum.py``).  The trainer
                                           # builds a ``GeodesicSpawner`` on the arena field (the shaper's, where both options are on) and
                                           # attaches it to its env: a slot whose episode ended respawns with every cop lo .. hi shortest-path hops
                                           # from a thief -- one launch of ``cat_render_nav_spawn`` and one masked ``cat_reset`` per tick inside
                                           # the captured rollout.  PRIVILEGED information reaches a policy only through where its episodes
                                           # start.  The random phase then runs tick by tick.  None: nothing is built, attached or launched
    curriculum_fraction: float = 1.0       # the first ``round(f N)`` slots take the band, the rest keep the map's own spawn
    curriculum_adapt: Optional[Tuple[float, float]] = None  # (low, high): ``update`` moves ``hi`` with the cops' win rate since the last update
                                           # (``GeodesicSpawner.adapt``): above ``high`` it rises by ``curriculum_step``, below ``low`` it falls
    curriculum_step: int = 1
    curriculum_max: int = 64               # the largest ``hi`` ``curriculum_adapt`` reaches

    def __post_init__(self):
        self._check_curriculum()
        k = self.frame_skip
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"TrainerConfig.frame_skip must be an integer >= 1, got {k!r}")
        for name in ("geodesic_shaping", "shaping_scale_thief"):
            v = getattr(self, name)
            if v is None and name == "shaping_scale_thief":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"TrainerConfig.{name} must be a finite number >= 0, got {v!r}")
        c = self.shaping_cap
        if isinstance(c, bool) or not isinstance(c, int) or not 1 <= c <= 65534:
            raise ValueError(f"TrainerConfig.shaping_cap must be an integer in 1 .. 65534, got {c!r}")

    def _check_curriculum(self) -> None:
        is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
        is_num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
        band = self.spawn_curriculum
        if band is not None:
            if not (isinstance(band, (tuple, list)) and len(band) == 2 and all(is_int(v) for v in band) and 1 <= band[0] <= band[1] <= 65534):
                raise ValueError(f"TrainerConfig.spawn_curriculum must be (lo, hi) with integers 1 <= lo <= hi <= 65534, got {band!r}")
            self.spawn_curriculum = (int(band[0]), int(band[1]))
        f = self.curriculum_fraction
        if not is_num(f) or not 0.0 <= f <= 1.0:
            raise ValueError(f"TrainerConfig.curriculum_fraction must be a number in 0 .. 1, got {f!r}")
        ad = self.curriculum_adapt
        if ad is not None:
            if not (isinstance(ad, (tuple, list)) and len(ad) == 2 and all(is_num(v) for v in ad) and 0.0 <= ad[0] <= ad[1] <= 1.0):
                raise ValueError(f"TrainerConfig.curriculum_adapt must be (low, high) with 0 <= low <= high <= 1, got {ad!r}")
            if band is None:
                raise ValueError("TrainerConfig.curriculum_adapt moves the band of spawn_curriculum, which is None")
            self.curriculum_adapt = (float(ad[0]), float(ad[1]))
        if not is_int(self.curriculum_step) or self.curriculum_step < 1:
            raise ValueError(f"TrainerConfig.curriculum_step must be an integer >= 1, got {self.curriculum_step!r}")
        if not is_int(self.curriculum_max) or not 1 <= self.curriculum_max <= 65534 or (band is not None and self.curriculum_max < band[1]):
            raise ValueError(f"TrainerConfig.curriculum_max must be an integer in 1 .. 65534 and at least the band's hi, got {self.curriculum_max!r}")

    @property
    def shaping_scales(self) -> Tuple[float, float]:
        """(cop scale, thief scale) of ``geodesic_shaping``; (0, 0) = off."""
        w = float(self.geodesic_shaping)
        return w, (w if self.shaping_scale_thief is None else float(self.shaping_scale_thief))


def compute_gae(rewards: torch.Tensor, values: torch.Tensor, dones: torch.Tensor, last_values: torch.Tensor,
                gamma: float, lam: float):
    """Reverse scan over the time axis (dim -2).  rewards/values: [..., T, N]; dones: [T, N] (the episode ended with
    tick t: no bootstrap across it); last_values: [..., N]."""
    T = rewards.shape[-2]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(last_values)
    nxt = last_values
    for t in range(T - 1, -1, -1):
        nd = 1.0 - dones[t].to(rewards.dtype)
        delta = rewards[..., t, :] + gamma * nxt * nd - values[..., t, :]
        last = delta + gamma * lam * nd * last
        adv[..., t, :] = last
        nxt = values[..., t, :]
    return adv, adv + values


def _rowsum(x: torch.Tensor) -> torch.Tensor:
    """x [G, ...] -> [G]: the sum over everything but the first axis, in stages of 256 so that every stage is a short
    inner-dimension reduction with many outputs.  Inside a captured HIP graph this replaces ``x.sum(dim=...)``: ``at::sum``
    of hundreds of thousands of elements into a few outputs is a MULTI-BLOCK reduction with a semaphore buffer, and
    replayed from a graph it returned garbage on this stack (ROCm 7.2 / torch 2.10) -- first for the bias gradients of the
    backward pass, then, at 8192 envs, for the validity check inside ``torch.multinomial`` (a spurious device-side
    assert).  Short reductions are done by one block per output and carry no such state."""
    flat = x.reshape(x.shape[0], -1)
    while flat.shape[1] > 2048:
        r = (-flat.shape[1]) % 256
        if r:
            flat = torch.nn.functional.pad(flat, (0, r))
        flat = flat.view(flat.shape[0], -1, 256).sum(-1)
    return flat.sum(-1)


def _sample(logp_all: torch.Tensor) -> torch.Tensor:
    """Categorical sample from log-probabilities [..., K] by inverse CDF on one uniform draw per row (elementwise ops and a
    K-term sum only; ``torch.multinomial``'s input validation is a large reduction, see ``_rowsum``)."""
    p = logp_all.exp()
    u = torch.rand(p.shape[:-1] + (1,), device=p.device, dtype=p.dtype)
    cdf = torch.cumsum(p, dim=-1)[..., :-1]
    return (u >= cdf).sum(dim=-1)


class _GradsOf(torch.autograd.Function):
    """A scalar whose gradient w.r.t. (logits, values) is the given pair: hooks the analytically computed gradient of
    the PPO loss (``cat_ppo_loss_grad``) into the autograd graph of the networks."""

    @staticmethod
    def forward(ctx, logits, values, d_logits, d_values):
        ctx.save_for_backward(d_logits, d_values)
        return logits.new_zeros(())

    @staticmethod
    def backward(ctx, g):
        d_logits, d_values = ctx.saved_tensors
        return d_logits, d_values, None, None


def _dist_ready() -> bool:
    """True when the optimiser step must all-reduce: a process group of more than one rank -- or of ONE rank with
    CAT_FORCE_ALLREDUCE=1, which sends the gradient buffer through the collective library anyway (the one-GPU test of the
    RCCL launch between the two step graphs)."""
    import os
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("CAT_FORCE_ALLREDUCE") == "1"


def advantage_moments(adv: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-agent mean and (unbiased) standard deviation of ``adv`` [G, T, N] over the WHOLE batch: with data-parallel ranks, over
    every rank's shard -- what one process holding all envs would normalise with (skrl: per agent, whole memory).  Two passes, as
    ``Tensor.std``: the mean first, then the squared deviations from it.  One rank: exactly ``adv.mean`` / ``adv.std``."""
    import torch.distributed as dist
    if not (_dist_ready() and dist.get_world_size() > 1):
        return adv.mean(dim=(1, 2), keepdim=True), adv.std(dim=(1, 2), keepdim=True)

    def total(t):
        if dist.get_backend() == "gloo" and t.is_cuda:
            host = t.cpu(); dist.all_reduce(host); return host.to(t.device)
        dist.all_reduce(t)
        return t
    n_local = float(adv.shape[1] * adv.shape[2])
    m1 = total(torch.stack([adv.sum(dim=(1, 2), dtype=torch.float64),
                            torch.full((adv.shape[0],), n_local, dtype=torch.float64, device=adv.device)]))
    n, mean64 = m1[1], m1[0] / m1[1]
    dev2 = total(((adv.double() - mean64.view(-1, 1, 1)) ** 2).sum(dim=(1, 2)))
    return mean64.float().view(-1, 1, 1), (dev2 / (n - 1)).sqrt().float().view(-1, 1, 1)


# ---------------------------------------------------------------------------------------------- running value normalisation
# ``cat_ppo_moments`` restated from include/cat_ppo.h in torch f64 on the CPU: every line is one IEEE operation on whole arrays, in the
# header's order, so the results are the kernel's bit for bit.  The learner's CPU path and the merge of the ranks' triples use them.
MOMENT_CHUNK = _learn_native.PPO_MOMENT_CHUNK       # CAT_PPO_MOMENT_CHUNK, the binding's one copy of it


def merge_moments(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """merge(a, b) of two f64 [..., 3] stacks of (n, mean, M2) triples (Chan et al., the header's order of operations)."""
    an, am, a2 = a.unbind(-1)
    bn, bm, b2 = b.unbind(-1)
    n = an + bn
    delta = bm - am
    w = bn / torch.where(n == 0, torch.ones_like(n), n)          # (n == 0 only where both are empty: a is returned there)
    mean = am + delta * w
    m2 = (a2 + b2) + (delta * delta) * (an * w)
    out = torch.stack([n, mean, m2], -1)
    out = torch.where((an == 0).unsqueeze(-1), b, out)
    return torch.where((bn == 0).unsqueeze(-1), a, out)


def running_moments(x: torch.Tensor) -> torch.Tensor:
    """x fp32 [G, M] -> f64 [G, 3] on the CPU: (n, mean, M2) of every row in ``cat_ppo_moments``'s order -- chunks of 4096, in a chunk
    256 "threads" that add their 16 strided elements left to right, a halving tree over the 256, the mean, the same again over the
    squared deviations; then a halving tree of ``merge_moments`` over the chunks, padded with empty triples to a power of two."""
    x = x.detach().to("cpu", torch.float64)
    G, M = x.shape
    chunks = -(-M // MOMENT_CHUNK)
    pad = chunks * MOMENT_CHUNK - M
    inside = torch.nn.functional.pad(torch.ones(M, dtype=torch.bool), (0, pad)).view(chunks, 16, 256)
    v = torch.nn.functional.pad(x, (0, pad)).view(G, chunks, 16, 256)         # [g][c][j][i] = x[g][c * 4096 + i + 256 j]

    def chunk_sum(e):           # elements out of range are +0.0: adding one leaves a sum that started at +0.0 as it is
        s = torch.zeros(G, chunks, 256, dtype=torch.float64)
        for j in range(16):
            s = s + e[:, :, j]
        stride = 128
        while stride:
            s = s[..., :stride] + s[..., stride:2 * stride]
            stride //= 2
        return s[..., 0]
    n = inside.sum(dim=(1, 2)).to(torch.float64).expand(G, chunks)
    mean = chunk_sum(v) / n
    d = torch.where(inside, v - mean.view(G, chunks, 1, 1), torch.zeros((), dtype=torch.float64))
    t = torch.stack([n, mean, chunk_sum(d * d)], -1)                           # [G, chunks, 3]
    P = 1
    while P < chunks:
        P *= 2
    t = torch.cat([t, torch.zeros(G, P - chunks, 3, dtype=torch.float64)], 1)
    while P > 1:
        P //= 2
        t = merge_moments(t[:, :P], t[:, P:2 * P])
    return t[:, 0]


def moments_scale(state: torch.Tensor) -> torch.Tensor:
    """f64 [G, 3] -> fp32 [G, 2] = (mu, sigma) = (mean, sqrt(M2 / n)), and (0, 1) while n == 0."""
    n, mean, m2 = state.unbind(-1)
    empty = n == 0
    sigma = torch.sqrt(m2 / torch.where(empty, torch.ones_like(n), n))
    return torch.stack([torch.where(empty, torch.zeros_like(mean), mean).float(), torch.where(empty, torch.ones_like(sigma), sigma).float()], -1)


# ---------------------------------------------------------------------------------------------- hyper-parameter schedules
# ``cat_ppo_schedule_step`` restated from include/cat_ppo.h on fp32 CPU tensors: every line is one rounded fp32 operation on whole arrays,
# in the header's order, so the block is the kernel's bit for bit.  The learner's CPU path runs it; the GPU path launches the kernel.
HYPER_STRIDE = _learn_native.PPO_HYPER_STRIDE
HYPER_LR, HYPER_ENTROPY, HYPER_RATIO_CLIP = _learn_native.HYPER_LR, _learn_native.HYPER_ENTROPY, _learn_native.HYPER_RATIO_CLIP
HYPER_KL_SUM, HYPER_KL_COUNT = _learn_native.HYPER_KL_SUM, _learn_native.HYPER_KL_COUNT
SCHED_KL, SCHED_ANNEAL = _learn_native.SCHED_KL, _learn_native.SCHED_ANNEAL
ANNEAL_LR, ANNEAL_ENTROPY, ANNEAL_RATIO_CLIP = _learn_native.ANNEAL_LR, _learn_native.ANNEAL_ENTROPY, _learn_native.ANNEAL_RATIO_CLIP


@torch.no_grad()
def schedule_step(hyper: torch.Tensor, sched_active: torch.Tensor, mode: int, *, kl_target: float = 0.008, kl_factor: float = 2.0,
                  lr_factor: float = 1.5, lr_min: float = 1e-6, lr_max: float = 1e-2, anneal_mask: int = 0, progress: float = 0.0,
                  lr=(0.0, 0.0), entropy=(0.0, 0.0), ratio_clip=(0.0, 0.0)) -> None:
    """``_learn_native.ppo_schedule_step`` on the CPU: ``hyper`` fp32 [G, 8] in place, ``sched_active`` fp32 [G]; same arguments, same checks."""
    assert hyper.dtype == torch.float32 and hyper.dim() == 2 and hyper.shape[1] == HYPER_STRIDE and hyper.device.type == "cpu"
    assert sched_active.dtype == torch.float32 and sched_active.shape == (hyper.shape[0],)
    f = lambda x: torch.tensor(x, dtype=torch.float32)          # a launch argument: the Python float rounded to fp32
    if mode not in (SCHED_KL, SCHED_ANNEAL, SCHED_KL | SCHED_ANNEAL):
        raise ValueError(f"schedule_step: mode must be 1..3, got {mode!r}")
    if not (f(lr_factor) >= 1 and f(kl_factor) >= 1 and f(lr_min) <= f(lr_max) and 0 <= f(progress) <= 1):
        raise ValueError("schedule_step: needs lr_factor >= 1, kl_factor >= 1, lr_min <= lr_max and progress in [0, 1]")
    if mode & SCHED_ANNEAL:
        for bit, col, (x0, x1) in ((ANNEAL_LR, HYPER_LR, lr), (ANNEAL_ENTROPY, HYPER_ENTROPY, entropy), (ANNEAL_RATIO_CLIP, HYPER_RATIO_CLIP, ratio_clip)):
            if anneal_mask & bit:
                d = f(x1) - f(x0)
                p = d * f(progress)
                hyper[:, col] = f(x0) + p
    if mode & SCHED_KL:
        hi = f(kl_target) * f(kl_factor)
        lo = f(kl_target) / f(kl_factor)
        count, old = hyper[:, HYPER_KL_COUNT], hyper[:, HYPER_LR]
        kl = hyper[:, HYPER_KL_SUM] / torch.where(count > 0, count, torch.ones_like(count))
        down = torch.maximum(old / f(lr_factor), f(lr_min))
        up = torch.minimum(old * f(lr_factor), f(lr_max))
        new = torch.where(kl > hi, down, torch.where(kl < lo, up, old))
        hyper[:, HYPER_LR] = torch.where((count > 0) & (sched_active != 0), new, old)
        hyper[:, HYPER_KL_SUM] = 0.0
        hyper[:, HYPER_KL_COUNT] = 0.0


class RoleLearner:
    """G agents that share one ``RoleConfig`` -- the agents of a role, or of both roles when the roles are configured
    alike (the reference's driver: ``CFG_AGENT`` for everyone) -- as stacked policy + value networks over one flat
    parameter buffer, with their Adam state, rollout buffers and PPO minibatch step.  Every launch then serves all of
    them: the update is bound by the number of kernels, not by their size."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-8    # torch.optim.Adam defaults (what skrl constructs)

    def __init__(self, role: str, agents: List[str], indices: List[int], R: int, N: int, T: int, cfg: RoleConfig,
                 device: torch.device, compute_dtype: torch.dtype, seeds: List[int], bptt: Optional[int] = None,
                 arch: str = "lstm", vwidth: Optional[int] = None, value_norm: bool = False):
        self.role, self.agents, self.indices, self.cfg = role, agents, indices, cfg
        self.agent_roles = [a.split("_")[0] for a in agents]
        self.G, self.R, self.N, self.T, self.device = len(agents), R, N, T, device
        self.bptt = bptt or T
        assert T % self.bptt == 0, "horizon must be a multiple of the BPTT window"
        self.W = T // self.bptt                                # windows per rollout; training sequences = W * N
        self.index_t = torch.tensor(indices, dtype=torch.long, device=device)     # columns of the [N, A] action tensor
        self.arch = arch
        self.fp = FlatParams(role_param_shapes(R, arch, vwidth), self.G, device, compute_dtype)
        init_from_modules(self.fp, R, seeds, arch, vwidth)
        self.policy, self.value = StackedNet("policy", R, self.fp, arch, vwidth), StackedNet("value", R, self.fp, arch, vwidth)
        G, P = self.G, self.fp.P
        f32 = dict(dtype=torch.float32, device=device)
        self.m, self.v, self.steps = torch.zeros(G, P, **f32), torch.zeros(G, P, **f32), torch.zeros(G, P, **f32)
        self.col_policy, self.col_value = self.fp.column_mask("policy."), self.fp.column_mask("value.")
        self.col_train = torch.ones(G, P, **f32)               # 1 where the parameter is trainable right now
        self.frozen = {r: [False, False] for r in set(self.agent_roles)}   # role -> [policy frozen, value frozen]
        self.epoch_active = torch.ones(G, **f32)               # KL early stop: 0 = skip the rest of this epoch
        self.ar = torch.zeros(G, P + 1, **f32)                 # all-reduce buffer: fp32 gradients | KL
        self.stat = torch.zeros(3, G, **f32)                   # last policy loss, value loss, KL per agent
        self._norm_scratch = torch.zeros(G, 256, **f32)
        self.native = self.device.type == "cuda" and compute_dtype == torch.bfloat16   # libcat_learn.so loss kernel
        W, S = self.W, self.W * N
        B = S // cfg.mini_batches
        if B < 1:
            raise ValueError(f"{S} training sequences ({W} BPTT windows x {N} envs on this rank) cannot fill {cfg.mini_batches} minibatches: "
                             "more envs per rank, a longer horizon or fewer minibatches")
        self.B = B
        self.idx = torch.zeros(B, dtype=torch.long, device=device)
        in_dt = dict(dtype=compute_dtype if self.native else torch.float32, device=device)   # the networks cast to it anyway
        self.buf = {"pin": torch.zeros(G, T, N, 2 * R, **in_dt), "vin": torch.zeros(G, T, N, self.value.in_width, **in_dt),
                    "act": torch.zeros(G, T, N, dtype=torch.long, device=device), "logp": torch.zeros(G, T, N, **f32),
                    "val": torch.zeros(G, T, N, **f32), "rew": torch.zeros(G, T, N, **f32),
                    "adv": torch.zeros(G, T, N, **f32), "ret": torch.zeros(G, T, N, **f32)}
        self.p_state = self.policy.initial_state(N)            # carried across rollouts
        self.v_state = self.value.initial_state(N)
        # recurrent states at the start of every window of the stored rollout: [W, layers, G, N, H]
        self.p0w = tuple(s.unsqueeze(0).repeat(W, 1, 1, 1, 1) for s in self.p_state)
        self.v0w = tuple(s.unsqueeze(0).repeat(W, 1, 1, 1, 1) for s in self.v_state)
        # what the minibatch step gathers from: [G, bptt, W * N, ...] (the rollout buffers themselves when W == 1)
        if W == 1:
            self.tb = self.buf
            self.p0, self.v0 = tuple(s[0] for s in self.p0w), tuple(s[0] for s in self.v0w)
            self.start = None                                  # set by update(): the trainer's [T, N] start flags
        else:
            self.tb = {k: torch.zeros((G, self.bptt, S) + tuple(v.shape[3:]), dtype=v.dtype, device=device)
                       for k, v in self.buf.items() if k not in ("val", "rew")}
            self.p0 = tuple(torch.zeros(s.shape[1], G, S, s.shape[4], dtype=s.dtype, device=device) for s in self.p0w)
            self.v0 = tuple(torch.zeros(s.shape[1], G, S, s.shape[4], dtype=s.dtype, device=device) for s in self.v0w)
            self.start = torch.zeros(self.bptt, S, dtype=torch.bool, device=device)
        self._graphs = None
        self.value_norm = value_norm
        if value_norm:      # TrainerConfig.value_norm: running moments of the raw returns and the scale the critic's targets are normalised with
            self.vn_state = torch.zeros(G, 3, dtype=torch.float64, device=device)              # (n, mean, M2) per agent
            self.vn_scale = torch.tensor([[0.0, 1.0]] * G, **f32)                              # (mu, sigma) per agent
            if self.native:
                self._vn_partial = torch.empty(G, _learn_native.ppo_moment_chunks(T * N), 3, dtype=torch.float64, device=device)
                self._vn_batch = torch.zeros(G, 3, dtype=torch.float64, device=device)
            self._vn_frozen = torch.zeros(G, 1, dtype=torch.bool, device=device)               # agents whose value network is frozen
        check_schedule(cfg)
        self.scheduled = scheduled(cfg)
        if self.scheduled:      # the learning rate, entropy scale and ratio clip of every agent live in device memory (include/cat_ppo.h: the hyper
            # block); the step kernels read them there, so the captured graphs follow the schedule rule without a recapture
            if G > _learn_native.SCHED_MAX_AGENTS:
                raise ValueError(f"a scheduled learner holds at most {_learn_native.SCHED_MAX_AGENTS} agents, not {G}")
            self.hyper = torch.zeros(G, HYPER_STRIDE, **f32)
            self.sched_active = torch.ones(G, **f32)           # 1 = the agent's policy is being trained (``set_frozen``)
            self.updates_done = 0                              # finished ``update`` calls: the linear anneals' clock
            self.anneal_mask = ((ANNEAL_LR if cfg.lr_schedule == "linear" else 0) | (ANNEAL_ENTROPY if cfg.entropy_final is not None else 0) |
                                (ANNEAL_RATIO_CLIP if cfg.ratio_clip_final is not None else 0))
            for g in range(G):
                self.set_schedule(g, None)

    # ------------------------------------------------------------------ hyper-parameter schedules
    def set_schedule(self, g: int, entry: Optional[dict]) -> None:
        """Agent g's row of the hyper block <- a checkpoint's ``"schedule"`` entry (None: the configured start values; the KL sums empty)."""
        cfg = self.cfg
        entry = entry or {}
        row = [0.0] * HYPER_STRIDE
        row[HYPER_LR] = float(entry.get("lr", cfg.learning_rate))
        row[HYPER_ENTROPY] = float(entry.get("entropy_scale", cfg.entropy_loss_scale))
        row[HYPER_RATIO_CLIP] = float(entry.get("ratio_clip", cfg.ratio_clip))
        self.hyper[g] = torch.tensor(row, dtype=torch.float32)
        self.updates_done = int(entry.get("updates", 0))       # one clock per learner: its agents' entries agree

    def schedule_entry(self, g: int) -> dict:
        """Agent g's current learning rate, entropy scale and ratio clip, and the learner's count of finished updates."""
        h = self.hyper[g].cpu()
        return {"lr": float(h[HYPER_LR]), "entropy_scale": float(h[HYPER_ENTROPY]), "ratio_clip": float(h[HYPER_RATIO_CLIP]),
                "updates": self.updates_done}

    def _schedule(self, mode: int, progress: float = 0.0) -> None:
        """One launch of the schedule rule on ``hyper`` (eager, between replays of the captured step graphs); on the CPU its restatement."""
        cfg = self.cfg
        step = _learn_native.ppo_schedule_step if self.device.type == "cuda" else schedule_step
        final = lambda x, x0: x0 if x is None else x
        step(self.hyper, self.sched_active, mode, kl_target=cfg.lr_kl_target, kl_factor=cfg.lr_kl_factor, lr_factor=cfg.lr_factor,
             lr_min=cfg.lr_min, lr_max=cfg.lr_max, anneal_mask=self.anneal_mask, progress=progress,
             lr=(cfg.learning_rate, final(cfg.lr_final, cfg.learning_rate)),
             entropy=(cfg.entropy_loss_scale, final(cfg.entropy_final, cfg.entropy_loss_scale)),
             ratio_clip=(cfg.ratio_clip, final(cfg.ratio_clip_final, cfg.ratio_clip)))

    # ------------------------------------------------------------------ freezing (skrl Model.freeze_parameters)
    def set_frozen(self, role: Optional[str] = None, policy: Optional[bool] = None, value: Optional[bool] = None) -> None:
        for r, fr in self.frozen.items():
            if role is None or r == role:
                if policy is not None:
                    fr[0] = policy
                if value is not None:
                    fr[1] = value
        rows = [self.col_policy * (0.0 if self.frozen[r][0] else 1.0) + self.col_value * (0.0 if self.frozen[r][1] else 1.0)
                for r in self.agent_roles]
        self.col_train.copy_(torch.stack(rows))
        if self.value_norm:     # a frozen critic keeps the scale it was trained under (``_moments_step``)
            self._vn_frozen.copy_(torch.tensor([[self.frozen[r][1]] for r in self.agent_roles]))
        if self.scheduled:      # a frozen policy has KL exactly 0: the KL rule leaves its learning rate alone
            self.sched_active.copy_(torch.tensor([0.0 if self.frozen[r][0] else 1.0 for r in self.agent_roles]))

    def rows(self, role: str) -> List[int]:
        return [g for g, r in enumerate(self.agent_roles) if r == role]

    # ------------------------------------------------------------------ the PPO minibatch step
    def _step_forward_backward(self) -> None:
        """zero grads, gather the minibatch ``self.idx`` (sequences = env slots), forward, losses, backward; leaves the
        fp32 gradients and the per-agent KL in ``self.ar``."""
        cfg, b, idx = self.cfg, self.tb, self.idx
        self.fp.grad.zero_()
        sel = lambda x: x.index_select(2, idx)
        keep = (~self.start.index_select(1, idx)).to(torch.float32)                    # [T, B]
        st = lambda s: s.index_select(2, idx)
        # the observations of the minibatch are read out of the rollout buffers in place (the fused trunk kernels take the index)
        logits, _ = self.policy.forward(b["pin"], (st(self.p0[0]), st(self.p0[1])), keep, select=idx)
        values, _ = self.value.forward(b["vin"], (st(self.v0[0]), st(self.v0[1])), keep, select=idx)
        M = float(logits.shape[1] * logits.shape[2])                                     # samples per agent in the minibatch
        ratio_clip, entropy_scale = cfg.ratio_clip, cfg.entropy_loss_scale
        if self.scheduled and not self.native:      # per agent, from the hyper block (fp32, as the kernel takes them)
            ratio_clip, entropy_scale = self.hyper[:, HYPER_RATIO_CLIP].view(-1, 1, 1), self.hyper[:, HYPER_ENTROPY]
        if self.native:   # loss, statistics and d loss / d (logits, values) in one launch (csrc/cat_ppo.hip)
            if self.scheduled:      # ... which reads the ratio clip and the entropy scale from the hyper block
                sums, d_logits, d_values = _learn_native.ppo_loss_grad_dev(
                    logits, values, sel(b["act"]), sel(b["logp"]), sel(b["adv"]), sel(b["ret"]), self.hyper, cfg.value_loss_scale)
            else:
                sums, d_logits, d_values = _learn_native.ppo_loss_grad(
                    logits, values, sel(b["act"]), sel(b["logp"]), sel(b["adv"]), sel(b["ret"]), cfg.ratio_clip, cfg.value_loss_scale,
                    cfg.entropy_loss_scale)
            policy_loss, value_loss, kl = -sums[:, 0] / M, cfg.value_loss_scale * sums[:, 1] / M, sums[:, 3] / M
            _GradsOf.apply(logits, values, d_logits, d_values).backward()
        else:
            logp_all = torch.log_softmax(logits.float(), dim=-1)                        # [G, T, B, 4]
            logp = logp_all.gather(-1, sel(b["act"]).unsqueeze(-1)).squeeze(-1)
            old = sel(b["logp"])
            ratio = torch.exp(logp - old)
            with torch.no_grad():
                kl = _rowsum((ratio - 1) - (logp - old)) / M                            # [G]
            adv = sel(b["adv"])
            surr = torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - ratio_clip, 1 + ratio_clip))
            policy_loss = -_rowsum(surr) / M
            entropy = -_rowsum((logp_all.exp() * logp_all).sum(-1)) / M
            value_loss = cfg.value_loss_scale * _rowsum((values.float().squeeze(-1) - sel(b["ret"])) ** 2) / M
            (policy_loss - entropy_scale * entropy + value_loss).sum().backward()   # agents share no parameter
        with torch.no_grad():
            self.ar[:, :-1].copy_(self.fp.grad)
            self.ar[:, -1].copy_(kl)
            self.stat[0].copy_(policy_loss); self.stat[1].copy_(value_loss)

    @torch.no_grad()
    def _step_apply(self) -> None:
        """KL gate, joint policy+value gradient-norm clip per agent, masked Adam, refresh of the compute copy."""
        cfg = self.cfg
        if self.device.type == "cuda" and self.scheduled:   # the learning rate from the hyper block; the KL sums of the epoch go there
            _learn_native.ppo_adam_step_dev(self.ar, self.col_train, self.epoch_active, self.m, self.v, self.steps, self.fp.master,
                                            None if self.fp.lp is self.fp.master else self.fp.lp, self.stat[2], self._norm_scratch,
                                            self.hyper, self.BETA1, self.BETA2, self.EPS, cfg.grad_norm_clip, cfg.kl_threshold)
            return
        if self.device.type == "cuda":   # the same step in two launches (csrc/cat_ppo.hip)
            _learn_native.ppo_adam_step(self.ar, self.col_train, self.epoch_active, self.m, self.v, self.steps, self.fp.master,
                                        None if self.fp.lp is self.fp.master else self.fp.lp, self.stat[2], self._norm_scratch,
                                        cfg.learning_rate, self.BETA1, self.BETA2, self.EPS, cfg.grad_norm_clip, cfg.kl_threshold)
            return
        kl = self.ar[:, -1]
        self.stat[2].copy_(kl)
        lr = cfg.learning_rate
        if self.scheduled:      # cat_ppo_adam_step_dev: an agent that enters the step active adds its KL to the epoch's sum
            was = self.epoch_active != 0
            self.hyper[:, HYPER_KL_SUM].add_(torch.where(was, kl, torch.zeros_like(kl)))
            self.hyper[:, HYPER_KL_COUNT].add_(was.to(torch.float32))
            lr = self.hyper[:, HYPER_LR].unsqueeze(1)
        if cfg.kl_threshold:
            self.epoch_active.mul_((kl <= cfg.kl_threshold).to(torch.float32))
        g = self.ar[:, :-1] * self.col_train                                           # frozen parameters: no gradient
        norm = _rowsum(g * g).sqrt().unsqueeze(1)
        g = g * torch.clamp(cfg.grad_norm_clip / (norm + 1e-6), max=1.0)                 # torch.nn.utils.clip_grad_norm_
        gate = self.epoch_active.unsqueeze(1) * self.col_train                         # [G, P]: 1 = this entry steps
        self.steps.add_(gate)
        self.m.add_(gate * (1 - self.BETA1) * (g - self.m))
        self.v.add_(gate * (1 - self.BETA2) * (g * g - self.v))
        s = self.steps.clamp_min(1.0)
        bc1, bc2 = 1 - self.BETA1 ** s, 1 - self.BETA2 ** s
        denom = (self.v / bc2).sqrt_().add_(self.EPS)
        self.fp.master.sub_(gate * lr * (self.m / bc1) / denom)
        self.fp.refresh()

    def minibatch_step(self, use_graph: bool) -> None:
        import torch.distributed as dist
        multi = _dist_ready()
        if use_graph and self._graphs is None:
            self._graphs = self._capture()
        if use_graph and self._graphs:
            self._graphs[0].replay()
        else:
            self._step_forward_backward()
        if multi:
            dist.all_reduce(self.ar, op=dist.ReduceOp.SUM)                             # RCCL over xGMI on a GPU node
            self.ar.div_(dist.get_world_size())
        if use_graph and self._graphs:
            self._graphs[1].replay()
        else:
            self._step_apply()

    def _capture(self):
        """Capture the two halves of the step in HIP graphs (``torch.cuda.CUDAGraph``).  Warm-up runs on a side stream
        first (library workspaces, autograd buffers), as whole-network capture requires; the optimiser state the warm-up
        touched is restored, so capturing does not train.  Returns () if the runtime refuses the capture."""
        kept = (self.fp.master, self.m, self.v, self.steps, self.epoch_active, self.ar, self.stat)
        if self.scheduled:      # the warm-up and the capture add to the KL sums of the hyper block
            kept += (self.hyper,)
        keep = [t.clone() for t in kept]

        def restore():
            for dst, src in zip(kept, keep):
                dst.copy_(src)
            self.fp.refresh()
        try:
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for _ in range(3):
                    self._step_forward_backward()
                    self._step_apply()
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            restore()
            ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga):
                self._step_forward_backward()
            with torch.cuda.graph(gb):
                self._step_apply()
            torch.cuda.synchronize(self.device)
            restore()
            return ga, gb
        except Exception as exc:   # noqa: BLE001 - keep training eagerly, but say so
            warnings.warn(f"HIP-graph capture of the {self.role} PPO step failed ({exc!r}); running it eagerly")
            torch.cuda.synchronize(self.device)
            restore()
            return ()

    # ------------------------------------------------------------------ running value normalisation
    def set_value_moments(self, g: int, triple: Optional[torch.Tensor]) -> None:
        """Agent g's running moments <- ``triple`` f64 [3] (None: a fresh scaler), and the scale they give."""
        self.vn_state[g] = 0.0 if triple is None else triple.to(self.device, torch.float64)
        self.vn_scale.copy_(moments_scale(self.vn_state.cpu()))

    @torch.no_grad()
    def _moments_step(self, raw: torch.Tensor) -> None:
        """The running moments take in this update's raw returns ``raw`` fp32 [G, M] (``_moments_merge``) -- but not those of an agent
        whose value network is frozen (``set_frozen(value=True)``): its critic is not trained meanwhile, so its outputs stay in the units
        of the scale it was trained under, and its ``vn_state`` / ``vn_scale`` rows stay as they are until it is released."""
        if not any(self.frozen[r][1] for r in self.agent_roles):
            return self._moments_merge(raw)
        state, scale = self.vn_state.clone(), self.vn_scale.clone()
        self._moments_merge(raw)
        self.vn_state.copy_(torch.where(self._vn_frozen, state, self.vn_state))
        self.vn_scale.copy_(torch.where(self._vn_frozen, scale, self.vn_scale))

    @torch.no_grad()
    def _moments_merge(self, raw: torch.Tensor) -> None:
        """``vn_state`` takes in the raw returns ``raw`` fp32 [G, M] of this update and ``vn_scale`` follows.  One rank on the kernel path:
        two launches of ``cat_ppo_moments``, no host involvement.  Several ranks: each takes the moments of its shard, the [G, 3] triples are
        all-gathered and every rank merges them into its state in rank order on the host -- the same operations on the same numbers, so all
        ranks keep bit-equal state (gloo takes CPU tensors, as in ``advantage_moments``)."""
        import torch.distributed as dist
        multi = _dist_ready() and dist.get_world_size() > 1
        if self.native and not multi:
            _learn_native.ppo_moments(raw, state=self.vn_state, scale_out=self.vn_scale, partial=self._vn_partial)
            return
        if self.native:
            _learn_native.ppo_moments(raw, batch_out=self._vn_batch, partial=self._vn_partial)
            batch = self._vn_batch
        else:
            batch = running_moments(raw)
        shards = [batch.cpu()]
        if multi:
            if dist.get_backend() == "gloo" or not batch.is_cuda:
                shards = [torch.empty_like(shards[0]) for _ in range(dist.get_world_size())]
                dist.all_gather(shards, batch.cpu())
            else:   # RCCL: device tensors.  (No test reaches this branch: the suite has gloo ranks on the CPU and one GPU.)
                shards = [torch.empty_like(batch) for _ in range(dist.get_world_size())]
                dist.all_gather(shards, batch.contiguous())
                shards = [t.cpu() for t in shards]
        state = self.vn_state.cpu()
        for t in shards:
            state = merge_moments(state, t)
        self.vn_state.copy_(state)
        self.vn_scale.copy_(moments_scale(state))

    def _scan_normalised(self, dones: torch.Tensor, last_values: torch.Tensor) -> torch.Tensor:
        """The update's first steps with ``value_norm``: the scan over the denormalised critic outputs (advantages and RAW returns), the
        running moments take the raw returns in, and ``buf["ret"]`` receives the returns normalised with the NEW scale.  Returns adv."""
        cfg, b, G = self.cfg, self.buf, self.G
        if self.native:
            adv, raw = torch.empty_like(b["adv"]), torch.empty_like(b["ret"])
            _learn_native.ppo_gae_scaled(b["rew"], b["val"], dones, last_values, self.vn_scale, cfg.discount_factor, cfg.gae_lambda, adv, raw)
        else:       # the header's two operations, then the plain recursion
            mu, sigma = self.vn_scale[:, 0].view(G, 1, 1), self.vn_scale[:, 1].view(G, 1, 1)
            adv, raw = compute_gae(b["rew"], b["val"] * sigma + mu, dones, last_values * sigma[:, 0] + mu[:, 0], cfg.discount_factor, cfg.gae_lambda)
        self._moments_step(raw.view(G, -1))
        mu, sigma = self.vn_scale[:, 0].view(G, 1, 1), self.vn_scale[:, 1].view(G, 1, 1)
        b["ret"].copy_((raw - mu) / (sigma + 1e-8))
        return adv

    # ------------------------------------------------------------------ update of one rollout
    def update(self, dones: torch.Tensor, starts: torch.Tensor, last_values: torch.Tensor, gen: torch.Generator,
               use_graph: bool) -> None:
        """dones/starts [T, N]; last_values [G, N] (bootstrap, already zeroed where the next tick starts an episode; with ``value_norm``
        a normalised critic output like ``buf["val"]``: the zero is then not a zero return, but ``dones`` of the last tick cuts it off)."""
        cfg, b = self.cfg, self.buf
        kl_rule = self.scheduled and cfg.lr_schedule == "kl_adaptive"
        if self.scheduled:
            if self.anneal_mask:    # the linear anneals: once per update, before its epochs
                self._schedule(SCHED_ANNEAL, min(1.0, self.updates_done / cfg.schedule_updates))
            if not kl_rule:         # nothing reads the KL sums the step kernel keeps: empty them, so that they stay small
                self.hyper[:, HYPER_KL_SUM:HYPER_KL_COUNT + 1].zero_()
        if self.value_norm:
            adv = self._scan_normalised(dones, last_values)
        elif self.native:   # the reverse scan over the T ticks as one launch (csrc/cat_ppo.hip) instead of ~7 small ones per tick
            adv = torch.empty_like(b["adv"])
            _learn_native.ppo_gae(b["rew"], b["val"], dones, last_values, cfg.discount_factor, cfg.gae_lambda, adv, b["ret"])
        else:
            adv, ret = compute_gae(b["rew"], b["val"], dones, last_values, cfg.discount_factor, cfg.gae_lambda)
            b["ret"].copy_(ret)
        mean, std = advantage_moments(adv)
        b["adv"].copy_((adv - mean) / (std + 1e-8))                                     # skrl: per agent, whole memory
        if self.W == 1:
            self.start = starts
        else:   # the rollout as W * N training sequences of ``bptt`` ticks: [G, W * bptt, N, ..] -> [G, bptt, W * N, ..]
            G, W, L, N = self.G, self.W, self.bptt, self.N
            for k, dst in self.tb.items():
                src = b[k]
                dst.copy_(src.view((G, W, L, N) + tuple(src.shape[3:])).transpose(1, 2).reshape(dst.shape))
            self.start.copy_(starts.view(W, L, N).transpose(0, 1).reshape(L, W * N))
            for dst, src in zip(self.p0 + self.v0, self.p0w + self.v0w):            # [W, layers, G, N, H] -> [layers, G, W * N, H]
                dst.copy_(src.permute(1, 2, 0, 3, 4).reshape(dst.shape))
        for _ in range(cfg.learning_epochs):
            self.epoch_active.fill_(1.0)
            perm = torch.randperm(self.W * self.N, generator=gen).to(self.device)
            for k in range(cfg.mini_batches):
                self.idx.copy_(perm[k * self.B:(k + 1) * self.B])
                self.minibatch_step(use_graph)
            if kl_rule:             # the epoch's mean KL moves every agent's learning rate; the sums start over
                self._schedule(SCHED_KL)
        if self.scheduled:
            self.updates_done += 1


class MAPPOTrainer:
    """MAPPO over a ``VecCopsEnv`` (or any env with its surface): roles ``cop`` and ``thief``."""

    def __init__(self, env, role_cfg: Optional[Dict[str, RoleConfig]] = None, trainer_cfg: Optional[TrainerConfig] = None,
                 device=None, seed: int = 0, split_roles: bool = False):
        """``split_roles``: one learner per role (keys "cop" and "thief") even where the roles are configured alike -- what
        ``set_opponent`` needs to hand one role to an actor.  The agents' initial weights do not depend on it."""
        self.env, self.tcfg = env, trainer_cfg or TrainerConfig()
        self.device = torch.device(device) if device is not None else getattr(env, "device", torch.device("cpu"))
        self.agents: List[str] = list(env.possible_agents)
        self.N = env.num_envs
        self.R = env.observation_spaces[self.agents[0]]["distance"].shape[0]
        role_cfg = role_cfg or {}
        n_cops = sum(a.startswith("cop") for a in self.agents)
        self.state_width = state_width(len(self.agents), n_cops, self.R)    # flattened shared state: the non-recurrent critic's input
        on_gpu = self.device.type == "cuda"
        dt = torch.bfloat16 if (self.tcfg.compute_bf16 and on_gpu) else torch.float32
        # roles configured alike are stacked into ONE learner (key "cop+thief"); otherwise one learner per role
        cfgs = {r: dataclasses.replace(role_cfg.get(r, CFG_AGENT)) for r in ("cop", "thief")
                if any(a.startswith(r) for a in self.agents)}
        groups: List[List[str]] = []
        for r in cfgs:
            for grp in groups:
                if cfgs[grp[0]] == cfgs[r] and not split_roles:
                    grp.append(r)
                    break
            else:
                groups.append([r])
        self.roles: Dict[str, RoleLearner] = {}
        for grp in groups:
            names = [a for a in self.agents if a.split("_")[0] in grp]
            idx = [self.agents.index(a) for a in names]
            self.roles["+".join(grp)] = RoleLearner("+".join(grp), names, idx, self.R, self.N, self.tcfg.horizon, cfgs[grp[0]],
                                                    self.device, dt, seeds=[seed * 1000 + i for i in idx],
                                                    bptt=min(self.tcfg.bptt, self.tcfg.horizon),
                                                    arch="lstm" if self.tcfg.recurrent else "mlp", vwidth=self.state_width,
                                                    **({"value_norm": True} if self.tcfg.value_norm else {}))
        for rl in self.roles.values():
            mask = [r in self.tcfg.random_action_roles for r in rl.agent_roles]
            rl.random_rows = torch.tensor(mask, device=self.device).view(rl.G, 1) if any(mask) else None
        R, d, t = self.R, 1.0 / 400.0, 0.25          # ray length (entity.py:176 default sensor), number of type codes - 1
        self._pin_scale = torch.tensor([d] * R + [t] * R, device=self.device)
        self._vin_scale = torch.tensor(([d] * R + [t] * R) * 2, device=self.device)
        nt = len(self.agents) - n_cops      # per agent (sorted ids: cops first): four ray channels, then its team's f16 positions (px)
        self._state_scale = torch.tensor(sum((([d] * R + [t] * R) * 2 + [1e-3] * (2 * (n_cops if i < n_cops else nt))
                                              for i in range(len(self.agents))), []), device=self.device)
        self._gen = torch.Generator(device="cpu").manual_seed(seed)
        torch.manual_seed(seed)
        self.timestep = 0
        self._obs, _ = env.reset()
        self._starts = torch.ones(self.N, dtype=torch.bool, device=self.device)
        self._keep32 = torch.zeros(1, self.N, dtype=torch.float32, device=self.device)   # = ~_starts, as the networks take it
        T = self.tcfg.horizon
        self._done_buf = torch.zeros(T, self.N, dtype=torch.bool, device=self.device)
        self._start_buf = torch.zeros(T, self.N, dtype=torch.bool, device=self.device)
        self._actions = torch.zeros(self.N, len(self.agents), dtype=torch.int32, device=self.device)
        self._native_io = on_gpu and hasattr(env, "raw_outputs") and self.tcfg.recurrent   # cat_rollout.h packs the LSTM pair's rows
        self._native_post = self._native_io and hasattr(env, "step_raw")   # cat_rollout_post: rewards and flags of the raw step   # cat_rollout.h: packing and sampling in one launch each
        self._graph = None
        self._graph_tables = ()                    # the opponent actors' league tables the captured rollout holds by value
        self._opponents: Dict[str, object] = {}    # learner key -> the actor that plays it (set_opponent)
        self._eager_rollouts = 0
        self._env_ticks = torch.zeros((), dtype=torch.int64, device=self.device)   # frame_skip > 1: summed from the env's ``ticks`` on the device
        self._env_ticks_host = 0                                                    # frame_skip == 1 and the fast-forward: N per tick, known here
        self.stats: Dict[str, float] = {}
        self.use_graphs = on_gpu
        self._collect_params: Dict[str, object] = {}    # fused_collect: learner key -> the kernel's parameter block (pointers into fp.lp)
        self._shapers: Dict[str, object] = {}      # geodesic_shaping: learner key -> its GeodesicShaper (all share one NavField)
        if any(self.tcfg.shaping_scales):
            self._build_shapers()
        self._spawner = None                       # spawn_curriculum: the GeodesicSpawner attached to the env
        self._curriculum_slots = slice(0, 0)
        if self.tcfg.spawn_curriculum is not None:
            self._build_spawner()
        if self.tcfg.fused_collect:
            self._check_fused_collect(on_gpu)

    def _build_spawner(self) -> None:
        """``TrainerConfig.spawn_curriculum``: a ``GeodesicSpawner`` on the arena field (the shapers' where there is one) over the first
        ``round(curriculum_fraction N)`` slots, attached to the env; the slots are then reset once more, so that the first episodes
        already start by the rule.  ValueError where the env cannot serve it."""
        from .curriculum import GeodesicSpawner
        if not hasattr(self.env, "set_spawner"):
            raise ValueError("spawn_curriculum needs an env with set_spawner() (VecCopsEnv)")
        lo, hi = self.tcfg.spawn_curriculum
        field = next((s.field for s in self._shapers.values()), None)
        self._curriculum_slots = slice(0, int(round(self.tcfg.curriculum_fraction * self.N)))
        self._spawner = GeodesicSpawner(self.env, lo, hi, field=field, slots=self._curriculum_slots)
        self.env.set_spawner(self._spawner)
        self._obs, _ = self.env.reset()

    def _build_shapers(self) -> None:
        """``TrainerConfig.geodesic_shaping``: per learner with a shaped agent a ``GeodesicShaper`` with the learner's own discount factor and
        a ``buf["shape"]`` [G, T, N] for the shaping terms (rows of agents left out stay 0).  ValueError where the env cannot serve it."""
        from .shaping import GeodesicShaper
        w_cop, w_thief = self.tcfg.shaping_scales
        field = None
        for key, rl in self.roles.items():
            shaper = GeodesicShaper(self.env, rl.agents, scale_cop=w_cop, scale_thief=w_thief, cap=self.tcfg.shaping_cap,
                                    gamma=rl.cfg.discount_factor, field=field)
            field = shaper.field
            if shaper.G:
                self._shapers[key] = shaper
                rl.buf["shape"] = torch.zeros(rl.G, self.tcfg.horizon, self.N, dtype=torch.float32, device=self.device)

    def _check_fused_collect(self, on_gpu: bool) -> None:
        """``TrainerConfig.fused_collect`` where the one-launch tick can never apply is an error, not a silent per-layer rollout."""
        tc, A = self.tcfg, len(self.agents)
        missing = []
        if not on_gpu:
            missing.append("a GPU (the device is %s)" % self.device)
        if not tc.compute_bf16:
            missing.append("bf16 compute (compute_bf16=False gives fp32)")
        if not tc.recurrent:
            missing.append("the recurrent policies (recurrent=False)")
        if not tc.deferred_values:
            missing.append("deferred_values=True")
        if tc.random_action_roles:
            missing.append(f"no random_action_roles (got {tuple(tc.random_action_roles)})")
        if not (hasattr(self.env, "raw_outputs") and hasattr(self.env, "step_raw")):
            missing.append("an env with raw_outputs() and step_raw()")
        if not (self.R in (64, 90) and all(_learn_native.act_supported(rl.G, self.N, A, self.R) for rl in self.roles.values())):
            missing.append(f"64 or 90 rays and at most {_learn_native.ACT_MAX_AGENTS} agents (the env has {self.R} rays, {A} agents): cat_act_supported")
        if missing:
            raise ValueError("TrainerConfig.fused_collect=True needs " + "; ".join(missing))

    def _collect_tick(self, key: str, rl: RoleLearner, t: int) -> None:
        """One policy-driven tick of learner ``rl`` in one launch: its rows of the rollout buffers at tick ``t``, its columns of the action matrix,
        its recurrent state in place and, at a window start, that state as it stood before the tick."""
        if key not in self._collect_params:          # the bf16 compute copy itself: every optimiser step is seen, also by a captured rollout
            self._collect_params[key] = _learn_native.act_params({n: rl.policy.w(n) for n in _learn_native.ACT_PARAM_NAMES})
        d, ts = (1.0 / 400.0, 0.25) if self.tcfg.normalize_inputs else (1.0, 1.0)
        b, (h, c) = rl.buf, rl.p_state
        k, first = divmod(t, rl.bptt)
        h0, c0 = (rl.p0w[0][k][0], rl.p0w[1][k][0]) if first == 0 else (None, None)
        u = torch.rand(rl.G, self.N, device=self.device)
        _learn_native.act_collect_step(self.env.raw_outputs(), rl.indices, self._collect_params[key], h[0], c[0], self._keep32, u, self._actions,
                                       sum(a.startswith("cop") for a in self.agents), self.tcfg.reference_q11, b["pin"][:, t], b["vin"][:, t],
                                       b["act"][:, t], b["logp"][:, t], h0, c0, d, ts)

    # ------------------------------------------------------------------ model inputs (packing.py layouts)
    def _pack_native(self, rl: RoleLearner, pin: torch.Tensor, vin: torch.Tensor) -> None:
        """The same rows as ``_inputs`` straight from the env core's buffers into bf16 ``pin`` / ``vin`` (one launch)."""
        d, t = (1.0 / 400.0, 0.25) if self.tcfg.normalize_inputs else (1.0, 1.0)
        _learn_native.rollout_pack(self.env.raw_outputs(), rl.indices, sum(a.startswith("cop") for a in self.agents),
                                   self.tcfg.reference_q11, d, t, pin, vin)

    def _inputs(self, rl: RoleLearner, obs, state) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._native_io and rl.native:
            pin = torch.empty(rl.G, self.N, 2 * self.R, dtype=torch.bfloat16, device=self.device)
            vin = torch.empty(rl.G, self.N, 4 * self.R, dtype=torch.bfloat16, device=self.device)
            self._pack_native(rl, pin, vin)
            return pin, vin
        pin = torch.stack([packing.pack_policy_input(obs[a]) for a in rl.agents])                       # [G, N, 2R]
        if not self.tcfg.recurrent:      # value_net.py: every agent's critic reads the whole flattened shared state
            vin = packing.pack_value_input(state).unsqueeze(0).expand(rl.G, -1, -1)
            if self.tcfg.normalize_inputs:
                pin, vin = pin * self._pin_scale, vin * self._state_scale
            return pin, vin
        first = sorted(state)[0]
        vin = torch.stack([packing.pack_agent_state(state[first if self.tcfg.reference_q11 else a])[:, :4 * self.R]
                           for a in rl.agents])                                                         # [G, N, 4R]
        if self.tcfg.normalize_inputs:   # channel layouts: [distance | type] and [distance_shared | type_shared | own distance | own type]
            pin, vin = pin * self._pin_scale, vin * self._vin_scale
        return pin, vin

    # ------------------------------------------------------------------ rollout
    def _rollout_ticks(self, random_actions) -> None:
        """T ticks: networks -> actions -> env.step into the preallocated buffers.  In-place updates of persistent
        tensors only and no host synchronisation: the whole loop is captured in one HIP graph and replayed.
        ``random_actions``: True / False for every learner, or the set of learner keys still in their ``random_timesteps``.
        With ``TrainerConfig.frame_skip`` k > 1 each of the T steps is a decision: the env plays up to k ticks with the actions held and
        returns the summed rewards, which go into the buffers as they come; the ticks played are added to a device counter."""
        N, T = self.N, self.tcfg.horizon
        skip = {} if self.tcfg.frame_skip == 1 else {"repeat": self.tcfg.frame_skip}     # 1: the call is today's, argument for argument
        learners = self.learners
        random_of = {key: (random_actions is True or (not isinstance(random_actions, bool) and key in random_actions))
                     for key in learners}
        any_random = any(random_of.values())
        all_fused = self._native_post and not any_random and all(rl.native and rl.random_rows is None for rl in learners.values())
        defer = all_fused and self._native_io and self.tcfg.deferred_values
        collect = self.tcfg.fused_collect and defer        # (defer implies all_fused: every learner is native and none acts at random)
        shapers = {key: self._shapers[key] for key in learners if key in self._shapers}
        for shaper in shapers.values():     # the separations of the state the rollout starts from, whatever happened to the env since the last
            shaper.prime(self.env.raw_outputs())       # one (reset, reset_episodes, load_state_dict, the random-phase fast-forward)
        for t in range(T):
            state = self.env.state()
            keep = self._keep32 if all_fused else (~self._starts).view(1, N)
            self._start_buf[t].copy_(self._starts)
            for key, rl in self.roles.items():
                if key in self._opponents:       # played by an actor: no network of the trainer runs, no rollout row is kept; the actor
                    # carries the role's recurrent state (zeroed where ``starts`` is set) and writes its columns of the action matrix
                    self._opponents[key].act(self.env, starts=self._starts, obs=self._obs, actions=self._actions)
                    continue
                if collect:
                    self._collect_tick(key, rl, t)
                    continue
                random_actions = random_of[key]
                if t % rl.bptt == 0:                # the recurrent state at the start of a BPTT window is kept
                    for dst, src in zip(rl.p0w + (() if defer else rl.v0w), rl.p_state + (() if defer else rl.v_state)):
                        dst[t // rl.bptt].copy_(src)
                b = rl.buf
                fused = self._native_io and rl.native and not random_actions and rl.random_rows is None
                if fused:   # rows packed straight into the rollout buffers; the networks read them there
                    pin, vin = b["pin"][:, t], b["vin"][:, t]
                    self._pack_native(rl, pin, vin)
                else:
                    pin, vin = self._inputs(rl, self._obs, state)
                logits, p_new = rl.policy.forward(pin.unsqueeze(1), rl.p_state, keep, update_state=True)
                if defer:                        # the critic runs after the last tick (below): no tick reads its value
                    val, v_new = None, rl.v_state
                else:
                    val, v_new = rl.value.forward(vin.unsqueeze(1), rl.v_state, keep, update_state=True)
                for old, new in zip(rl.p_state + rl.v_state, p_new + v_new):
                    if old is not new:           # the kernel path has already written the new state in place
                        old.copy_(new)
                if fused:   # draw, log-probability, value and the env's action columns in one launch
                    u = torch.rand(rl.G, N, device=self.device)
                    _learn_native.rollout_sample(logits[:, 0].contiguous(), u, None if defer else val[:, 0, :, 0].contiguous(), b["act"][:, t],
                                                 b["logp"][:, t], None if defer else b["val"][:, t], self._actions, rl.indices)
                    continue
                logp_all = torch.log_softmax(logits[:, 0].float(), dim=-1)                               # [G, N, 4]
                if random_actions:
                    act = torch.randint(0, 4, (rl.G, N), generator=self._gen).to(self.device)
                else:
                    act = _sample(logp_all)
                    if rl.random_rows is not None:   # rows of the roles in TrainerConfig.random_action_roles
                        act = torch.where(rl.random_rows, torch.randint(0, 4, (rl.G, N), device=self.device), act)
                b["pin"][:, t].copy_(pin); b["vin"][:, t].copy_(vin); b["act"][:, t].copy_(act)
                b["logp"][:, t].copy_(logp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1))
                b["val"][:, t].copy_(val[:, 0, :, 0].float())
                self._actions.index_copy_(1, rl.index_t, act.t().to(torch.int32))    # device index: capturable
            if all_fused:   # one launch for the tick, one for rewards + episode-end flags (cat_rollout_post)
                raw = self.env.step_raw(self._actions, **skip)
                if skip:
                    self._env_ticks.add_(raw["ticks"].sum())
                for i, (key, rl) in enumerate(learners.items()):
                    flags = (self._done_buf[t], self._starts, self._keep32) if i == 0 else (None, None, None)
                    _learn_native.rollout_post(raw, rl.indices, rl.buf["rew"][:, t], *flags)
                    if key in shapers:             # rew += F, shape = F: one launch, after the rewards of the tick are in place
                        shapers[key].step(raw, rl.buf["rew"][:, t], rl.buf["shape"][:, t])
                self._obs = self.env.observations()
                continue
            self._obs, rewards, terms, truncs, infos = self.env.step(self._actions, **skip)
            if skip:
                self._env_ticks.add_(infos["ticks"].sum())
            done = terms[self.agents[0]]
            for key, rl in learners.items():
                rl.buf["rew"][:, t].copy_(torch.stack([rewards[a].float() for a in rl.agents]))
                if key in shapers:
                    shapers[key].step(self.env.raw_outputs(), rl.buf["rew"][:, t], rl.buf["shape"][:, t])
            self._done_buf[t].copy_(done)
            self._starts.copy_(done)               # the env auto-resets: the next tick starts a new episode
            self._keep32.copy_((~done).view(1, N))
        if defer:
            # The critics, one BPTT window at a time over the stored input rows: 16 ticks x N envs per launch instead of N, the
            # recurrence of a window in one launch per layer, and the window-start states fall out on the way.  (The cell state
            # stays fp32 inside a window, as in the training forward, where tick-by-tick it is rounded to bf16 every tick.)
            keep_all = (~self._start_buf).to(torch.float32)
            for rl in learners.values():
                L = rl.bptt
                for k in range(rl.W):
                    for dst, src in zip(rl.v0w, rl.v_state):
                        dst[k].copy_(src)
                    val, _ = rl.value.forward(rl.buf["vin"][:, k * L:(k + 1) * L], rl.v_state, keep_all[k * L:(k + 1) * L], update_state=True)
                    rl.buf["val"][:, k * L:(k + 1) * L].copy_(val[..., 0])

    @torch.no_grad()
    def collect(self, random_actions=False) -> None:
        """One rollout of ``horizon`` ticks into the role buffers (``random_actions``: see ``_rollout_ticks``)."""
        random_actions = random_actions if isinstance(random_actions, bool) else (frozenset(random_actions) or False)
        use_graph = self.tcfg.graph_rollout and self.use_graphs and not random_actions and self._opponents_capturable()
        if self._graph is not None and self._graph_tables != self._opponent_tables():
            self._graph = None                      # set_matchups since the capture: the graph holds the old table by value
        if not use_graph:
            self._rollout_ticks(random_actions)
            self._eager_rollouts += 0 if random_actions else 1
        else:
            if self._graph is None:
                if self._eager_rollouts == 0:       # the first policy-driven rollout runs eagerly: every op of the tick
                    self._rollout_ticks(False)      # (sampling included) has then run once before it is captured
                    self._eager_rollouts += 1
                    self.timestep += self.tcfg.horizon
                    self._count_env_ticks(self.tcfg.horizon)
                    return
                torch.cuda.synchronize(self.device)
                self._graph = torch.cuda.CUDAGraph()
                self._graph_tables = self._opponent_tables()
                with torch.cuda.graph(self._graph):
                    self._rollout_ticks(False)
            self._graph.replay()
        self.timestep += self.tcfg.horizon
        self._count_env_ticks(self.tcfg.horizon)

    # ------------------------------------------------------------------ roles played by an actor
    @property
    def learners(self) -> Dict[str, RoleLearner]:
        """The learners the trainer itself plays and trains: all of ``roles`` but those handed to an actor by ``set_opponent``."""
        return {k: rl for k, rl in self.roles.items() if k not in self._opponents}

    def _opponent_tables(self) -> tuple:
        return tuple(getattr(a, "table", None) for a in self._opponents.values())

    def _opponents_capturable(self) -> bool:
        """Only the one-launch kernel of a fused actor belongs in a captured rollout: the per-layer chain copies from the host for a "random"
        agent, and it reads per-segment copies of the bank that ``load_set`` frees and rebuilds."""
        return all(getattr(a, "fused", False) for a in self._opponents.values())

    def set_opponent(self, role_key: str, actor) -> None:
        """Hand the learner ``role_key`` (a key of ``roles``) to ``actor`` (``actor.LeagueActor.from_env(env, sets, agents=<that learner's
        agents>)`` over this trainer's env), or take it back with ``actor=None``.  While set, the rollout asks the actor for that role's
        action columns (``actor.act(env, starts=..., actions=<the trainer's action matrix>)``), evaluates none of the role's networks and
        keeps no rollout row of it; ``update`` / ``train`` never touch it (its parameters and Adam state stay bit-unchanged), and
        ``read_stats``, ``state_dict`` and ``param_digest`` leave it out.  The role's recurrent state lives in the actor.

        The rollout stays ONE captured graph.  Fixed by a capture: the actor's league table (a launch argument, copied by value) and the
        addresses of the bank, of the actor's state and of the action matrix.  NOT fixed: the bank's contents -- ``actor.load_set`` between
        replays reaches the next replay without a recapture.  Setting or clearing an opponent drops the captured graph, and ``collect``
        recaptures when it finds that ``set_matchups`` has replaced the table since.

        All of that holds for a FUSED actor (``actor.fused``: a GPU, bf16, recurrent policies, 64 or 90 rays).  With an unfused actor -- the
        CPU, or a GPU where the kernel does not apply and the actor fell back to its per-layer chain -- nothing is captured: every rollout
        runs eagerly for as long as that actor is set, whatever ``graph_rollout`` says, so ``load_set`` and ``set_matchups`` take effect
        there too.

        One role at a time: at least one learner stays with the trainer, which with the two roles leaves room for ONE opponent actor."""
        if role_key not in self.roles:
            raise ValueError(f"{role_key!r} is not a learner of this trainer: {sorted(self.roles)}")
        if actor is None:
            if self._opponents.pop(role_key, None) is not None:
                for st in self.roles[role_key].p_state + self.roles[role_key].v_state:
                    st.zero_()                     # the trainer's own state of the role did not follow the episodes meanwhile
        else:
            rl = self.roles[role_key]
            if list(getattr(actor, "agents", ())) != list(rl.agents):
                raise ValueError(f"the actor must cover exactly the agents {rl.agents} of learner {role_key!r}, not {list(getattr(actor, 'agents', ()))}")
            if getattr(actor, "N", None) != self.N or list(getattr(actor, "env_agents", ())) != self.agents:
                raise ValueError(f"the actor must be built over this trainer's env ({self.N} envs, agents {self.agents})")
            if torch.device(actor.device).type != self.device.type:
                raise ValueError(f"the actor lies on {actor.device}, the trainer on {self.device}")
            if len(self.learners) - (role_key in self.learners) < 1:
                raise ValueError("at least one learner must stay with the trainer")
            self._opponents[role_key] = actor
        self._graph, self._graph_tables = None, ()
        self._eager_rollouts = 0                   # the next policy-driven rollout runs eagerly once more before the capture

    def _count_env_ticks(self, ticks: int) -> None:
        """``ticks`` one-tick steps of all N slots went by (with ``frame_skip`` > 1 the rollout counts on the device instead)."""
        if self.tcfg.frame_skip == 1:
            self._env_ticks_host += self.N * ticks

    # ------------------------------------------------------------------ update
    def update(self, only: Optional[Sequence[str]] = None) -> Dict[str, float]:
        """PPO update of every learner (or of the learner keys in ``only``) from the rollout just collected."""
        N = self.N
        todo = {k: rl for k, rl in self.learners.items() if only is None or k in only}
        if self.tcfg.check_device_errors:
            # the env ticks of the rollout were asynchronous launches that cannot raise: read the device error word once per update (one stream
            # synchronisation, where the rollout has to be complete anyway) -- a bad action, a dropped contact or a scheduler fault stops training
            # here, as the reference's exceptions would (entity.py:126-134)
            check = getattr(self.env, "check_errors", None)   # (the CPU test doubles of the env have no device)
            if check is not None:
                check()
        if self._spawner is not None and self.tcfg.curriculum_adapt is not None:     # (the stream is synchronised just above)
            low, high = self.tcfg.curriculum_adapt
            self._spawner.adapt(low, high, self.tcfg.curriculum_step, hi_max=self.tcfg.curriculum_max)
        with torch.no_grad():
            state = self.env.state()
            keep = (~self._starts).view(1, N)
            last = {}
            for role, rl in todo.items():
                _, vin = self._inputs(rl, self._obs, state)
                val, _ = rl.value.forward(vin.unsqueeze(1), tuple(s.clone() for s in rl.v_state), keep)
                last[role] = val[:, 0, :, 0].float() * (~self._starts).float()
        use_graph = self.tcfg.graph_update and self.use_graphs
        for role, rl in todo.items():
            rl.update(self._done_buf, self._start_buf, last[role], self._gen, use_graph)
        return {}

    def read_stats(self) -> Dict[str, float]:
        """Host copy of the last minibatch's losses (one synchronisation; call it when you want to look), and ``env_ticks``: the env
        ticks (slot-ticks, summed over the batch) played by ``collect`` and the random-phase fast-forward since the trainer was built --
        with ``frame_skip`` > 1 the device sum of the env's per-slot ``ticks``, read here and nowhere else."""
        out = {}
        for rl in self.learners.values():
            s = rl.stat.cpu()
            for g, a in enumerate(rl.agents):
                out[f"{a}/policy_loss"], out[f"{a}/value_loss"], out[f"{a}/kl"] = float(s[0, g]), float(s[1, g]), float(s[2, g])
            if rl.value_norm:           # the scale the critic's targets are normalised with: (0, 1) before the first update
                sc = rl.vn_scale.cpu()
                for g, a in enumerate(rl.agents):
                    out[f"value_mean/{a}"], out[f"value_std/{a}"] = float(sc[g, 0]), float(sc[g, 1])
            if rl.scheduled:            # what the next minibatch step would train with
                h = rl.hyper.cpu()
                for g, a in enumerate(rl.agents):
                    out[f"lr/{a}"], out[f"entropy_scale/{a}"], out[f"ratio_clip/{a}"] = (float(h[g, HYPER_LR]), float(h[g, HYPER_ENTROPY]),
                                                                                       float(h[g, HYPER_RATIO_CLIP]))
        for key, shaper in self._shapers.items():
            if key in self._opponents:
                continue
            rl = self.roles[key]
            mean_f = rl.buf["shape"].mean(dim=(1, 2)).cpu()                # the last rollout's shaping terms
            hops = shaper.hops_prev.cpu()
            for g, a in zip(shaper.rows, shaper.agents):
                out[f"shaping/{a}"] = float(mean_f[g])
            for row, a in zip(hops, shaper.agents):                        # the separations the next rollout starts from, where defined
                out[f"geodesic_hops/{a}"] = float(row[row >= 0].float().mean()) if bool((row >= 0).any()) else float("nan")
        if self._spawner is not None:      # with curriculum_adapt: the counters the last update's adapt read; else everything since the start
            sp = self._spawner
            c = sp.last if (self.tcfg.curriculum_adapt is not None and sp.last is not None) else sp.counters()
            out["curriculum/hi"] = sp.hi
            out["curriculum/cop_win_rate"] = c["cop_wins"] / c["ended"] if c["ended"] else float("nan")
            out["curriculum/placed"], out["curriculum/fallbacks"] = c["placed_total"], c["requested"] - c["placed_total"]
        ep = self._episode_stats()
        if ep is not None:
            e = ep()
            out["episodes"], out["cop_win_rate"], out["mean_episode_length"] = e["episodes"], e["cop_win_rate"], e["mean_length"]
            for a in self.agents:
                out[f"mean_return/{a}"] = e[f"mean_return/{a}"]
            actor = next(iter(self._opponents.values()), None)    # at most one: set_opponent keeps a learner, and there are two roles
            if actor is not None:                    # per opponent segment: EpisodeTracker.segment_summary
                bounds = [lo for lo, _ in actor.segments] + [self.N]
                out["segments"] = self.env.episode_tracker.segment_summary(bounds)
        out["env_ticks"] = self._env_ticks_host + int(self._env_ticks)
        self.stats = out
        return out

    def _episode_stats(self):
        """The env's ``episode_stats`` when ``TrainerConfig.episode_stats`` asks for it and the env offers it, else None."""
        return getattr(self.env, "episode_stats", None) if self.tcfg.episode_stats else None

    def set_frozen(self, role: Optional[str] = None, policy: Optional[bool] = None, value: Optional[bool] = None) -> None:
        for rl in self.roles.values():
            rl.set_frozen(role, policy, value)

    def learner_of(self, agent: str) -> Tuple[RoleLearner, int]:
        for rl in self.roles.values():
            if agent in rl.agents:
                return rl, rl.agents.index(agent)
        raise KeyError(agent)

    def train(self, timesteps: Optional[int] = None, freeze_policies_first: bool = True) -> Dict[str, float]:
        """One ``SequentialTrainer.train()`` of the reference's simultaneous mode (``agent_learning_utils.py:172-197``):
        the timestep restarts at 0, every policy starts frozen and every value network trainable, and the durations of
        ``CFG_TRAINER`` release them."""
        tc = self.tcfg
        timesteps = tc.timesteps if timesteps is None else timesteps
        self.timestep = 0
        ep = self._episode_stats()
        if ep is not None:
            self.env.episode_tracker.clear()                     # the figures of read_stats describe this call
        if freeze_policies_first:
            self.set_frozen(policy=tc.policy_freeze_duration > 0, value=False)
        while self.timestep < timesteps:
            t0, t1 = self.timestep, self.timestep + tc.horizon
            span = self._random_phase_span(t0, timesteps)
            if span:
                t1 = t0 + span
            if tc.opponent_freeze_duration > 0 and t0 <= tc.opponent_freeze_duration < t1:
                self.set_frozen(value=False)                     # "Unfreezing opponent agent" (README.md:104-108)
            if tc.policy_freeze_duration > 0 and t0 <= tc.policy_freeze_duration < t1:
                self.set_frozen(policy=False)                    # "Unfreezing policy network" (:109-113)
            # skrl keeps these two thresholds per agent (each agent's own cfg): a learner still inside its random_timesteps
            # acts uniformly at random while another already samples its policy, and each starts updating on its own
            if span:            # every learner acts at random and nothing of these ticks is kept: one resident launch
                self._fast_forward_random(span)
                continue
            in_random = frozenset(k for k, rl in self.learners.items() if t0 < rl.cfg.random_timesteps)
            self.collect(random_actions=in_random)
            # skrl updates an agent whenever its timestep has reached ITS learning_starts, whatever its random_timesteps (a config
            # with learning_starts below random_timesteps trains on uniformly random transitions, as in the reference's stack)
            ready = [k for k, rl in self.learners.items() if self.timestep >= rl.cfg.learning_starts]
            if ready:
                self.update(only=None if len(ready) == len(self.learners) else ready)
        return self.read_stats()

    def _random_phase_span(self, t0: int, timesteps: int) -> int:
        """How many ticks from ``t0`` can run as ONE resident random-action launch: whole rollouts (thresholds act at rollout
        granularity, as in the tick-by-tick path) during which every learner is inside its ``random_timesteps`` and after which none
        is due an update.  0: take the ordinary path."""
        tc = self.tcfg
        if not (tc.resident_random_phase and hasattr(self.env, "rollout_random")) or tc.random_action_roles or self._opponents:
            return 0                                 # (an opponent actor plays its policies during the learner's random phase too)
        if self._spawner is not None:
            return 0                                 # (the resident launch cannot respawn between its ticks: the phase runs tick by tick)
        H = tc.horizon
        end = min(rl.cfg.random_timesteps for rl in self.roles.values())
        first_update = min(rl.cfg.learning_starts for rl in self.roles.values())
        n = 0
        # rollout n starts at t0 + n H inside EVERY learner's random phase (no network is consulted for an action) and ends before
        # any learner's learning_starts (no update follows it, so nothing of it is ever read)
        while t0 + (n + 1) * H <= timesteps and t0 + n * H < end and t0 + (n + 1) * H < first_update:
            n += 1
        return n * H

    def _fast_forward_random(self, ticks: int) -> None:
        self._synth_tick = getattr(self, "_synth_tick", 1 << 20)
        out = self.env.rollout_random(ticks, tick0=self._synth_tick)
        self._synth_tick += ticks
        self._obs = self.env.observations()
        done = out["terminated"].bool()
        self._starts.copy_(done)                      # the env auto-resets: the next tick starts a new episode there
        self._keep32.copy_((~done).view(1, self.N))
        for rl in self.roles.values():                # no network ran during the phase: the recurrent states start from zero
            for st in rl.p_state + rl.v_state:
                st.zero_()
        self.timestep += ticks
        self._env_ticks_host += self.N * ticks      # one-tick steps whatever frame_skip is: nothing decides during this phase

    # ------------------------------------------------------------------ checkpoints
    def agent_models(self, agent: str) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"policy": sd, "value": sd} with the reference modules' parameter names (models.LSTMPolicy / LSTMValue)."""
        rl, g = self.learner_of(agent)
        return agent_state_dict(rl.fp, g)

    META_KEY = "__cat__"     # trainer position; not an agent name, so skrl's ``MAPPO.load`` (which walks possible_agents) skips it

    def state_dict(self) -> dict:
        """The "full agent" in the layout skrl's ``MAPPO.save`` writes ([SKRL-RECALL] ``{agent: {"policy": state_dict,
        "value": state_dict, "optimizer": Adam.state_dict()}}``; the reference saves it as ``joint_iter_N_full_agent.pt``,
        agent_learning_utils.py:263) with the reference modules' parameter names, plus the trainer position under
        ``__cat__``.  Everything is stored per agent, so a checkpoint does not depend on how the agents were stacked."""
        out = {}
        for a in self.agents:
            rl, g = self.learner_of(a)
            if rl.role in self._opponents:           # played by an actor (set_opponent): not this trainer's to save
                continue
            sched = rl.schedule_entry(g) if rl.scheduled else None
            out[a] = dict(self.agent_models(a), optimizer=adam_state_dict(rl.fp, g, rl.m, rl.v, rl.steps,
                                                                         sched["lr"] if sched else rl.cfg.learning_rate,
                                                                         (rl.BETA1, rl.BETA2), rl.EPS))
            if sched:                   # the agent's current learning rate, entropy scale and ratio clip, and the anneals' clock
                out[a]["schedule"] = sched
            if rl.value_norm:           # the running moments the agent's critic was trained under: (n, mean, M2), f64
                out[a]["vn_state"] = rl.vn_state[g].detach().cpu().clone()
        out[self.META_KEY] = {"format": "cat-mappo-3", "timestep": self.timestep, "num_rays": self.R, "recurrent": bool(self.tcfg.recurrent)}
        if self._spawner is not None:   # where the start-state curriculum stands
            out[self.META_KEY]["curriculum"] = {"lo": self._spawner.lo, "hi": self._spawner.hi}
        return out

    def load_state_dict(self, sd: dict, roles: Optional[List[str]] = None, optimizer: bool = True) -> None:
        """``roles``: restrict to these roles' models (reference ``copy_role_models``, which copies policy and value
        weights only: pass ``optimizer=False`` for that).  Accepts this class's checkpoints, a checkpoint written by the
        reference (skrl layout, no ``__cat__``; preprocessor entries are ignored, the reference configures none) and
        round-2 files (``{"format": "cat-mappo-2", "models": ..., "optimizers": ...}``).  A scheduled learner (``RoleConfig.lr_schedule`` ...)
        takes an agent's ``schedule`` entry (none: it starts from the config); a trainer without schedules ignores them with one warning.  With ``TrainerConfig.value_norm`` an agent's
        ``vn_state`` is restored with its models (an agent entry without one starts a fresh scaler); without the option a checkpoint's
        ``vn_state`` entries are ignored with one warning."""
        if sd.get("format") == "cat-mappo-2":
            sd = dict({a: dict(sd["models"][a], **({"optimizer": sd["optimizers"][a]} if a in sd.get("optimizers", {}) else {}))
                       for a in sd["models"]}, **{self.META_KEY: {"timestep": sd.get("timestep", 0)}})
        ignored: List[str] = []
        unscheduled: List[str] = []
        for a in self.agents:
            if roles is not None and a.split("_")[0] not in roles:
                continue
            if a not in sd:
                raise KeyError(f"checkpoint holds no agent {a!r} (it has {sorted(k for k in sd if k != self.META_KEY)})")
            rl, g = self.learner_of(a)
            load_agent_state_dict(rl.fp, g, sd[a])
            if optimizer and "optimizer" in sd[a]:
                load_adam_state_dict(rl.fp, g, rl.m, rl.v, rl.steps, sd[a]["optimizer"])
            if rl.value_norm:           # goes with the value network: its outputs are in these units.  No entry: a fresh scaler
                rl.set_value_moments(g, sd[a].get("vn_state"))
            elif "vn_state" in sd[a]:
                ignored.append(a)
            if not optimizer:           # the schedule goes with the optimiser: a copy of the models alone leaves it as it is
                pass
            elif rl.scheduled:          # no entry: the schedule starts from the config
                rl.set_schedule(g, sd[a].get("schedule"))
            elif "schedule" in sd[a]:
                unscheduled.append(a)
        if unscheduled:
            warnings.warn(f"the checkpoint holds scheduled hyper-parameters (schedule) of {unscheduled}, which a trainer without schedules ignores: "
                          "it trains them at its configured learning rate, entropy scale and ratio clip")
        if ignored:
            warnings.warn(f"the checkpoint holds running value moments (vn_state) of {ignored}, which a trainer with value_norm=False ignores: "
                          "their value networks were trained on normalised returns")
        if optimizer and roles is None:
            self.timestep = int(sd.get(self.META_KEY, {}).get("timestep", 0))
        cur = sd.get(self.META_KEY, {}).get("curriculum") if roles is None else None    # (a copy of one role's models leaves the band alone)
        if cur is not None and self._spawner is not None:
            self._spawner.set_band(int(cur["lo"]), int(cur["hi"]), self._curriculum_slots)
        elif cur is not None:
            warnings.warn(f"the checkpoint holds a start-state curriculum (lo {cur['lo']}, hi {cur['hi']}), which a trainer with "
                          "spawn_curriculum=None ignores: its episodes start where the map's spawn rule puts them")

    def param_digest(self) -> str:
        """SHA-256 over every learner's fp32 master parameters and optimiser step counts: data-parallel replicas must agree on it."""
        import hashlib
        h = hashlib.sha256()
        for k in sorted(self.learners):
            rl = self.roles[k]
            h.update(rl.fp.master.detach().float().cpu().numpy().tobytes())
            h.update(rl.steps.detach().cpu().numpy().tobytes())
        return h.hexdigest()

    def reset_optimizers(self) -> None:
        """A fresh Adam, as every self-play iteration of the reference constructs a new ``MAPPO`` (orchestration.py:135-144)."""
        for rl in self.roles.values():
            rl.m.zero_(); rl.v.zero_(); rl.steps.zero_()

    def reset_episodes(self) -> None:
        """Restart every env slot and the recurrent states (after an evaluation used the same env, or on resume)."""
        self._obs, _ = self.env.reset()
        self._starts.fill_(True)
        self._keep32.zero_()
        for rl in self.roles.values():
            for s in rl.p_state + rl.v_state:
                s.zero_()
        for actor in self._opponents.values():
            actor.reset()
