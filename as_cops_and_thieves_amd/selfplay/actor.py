"""Inference-only policy actor: everything that PLAYS trained policies -- watching a checkpoint, the evaluation protocol, the PFSP
evaluation of the self-play loop -- needs the policies' parameters, their recurrent state and a way from the env's observations to its
action matrix, and nothing else of a ``MAPPOTrainer`` (no critics, no optimiser state, no ``[G, T, N, ...]`` rollout buffers).

    actor = PolicyActor.from_checkpoint("run/joint_iter_3_full_agent.pt", env)      # or {"cop": file_a, "thief": file_b}
    actor.reset()
    actions = actor.act(env, starts)            # [N, A] int32, a persistent buffer: env.step(actions)

Two back ends, chosen by ``fused``:

* fused (``True``: a GPU, bf16, the recurrent pair with 64 or 90 rays, an env that offers ``raw_outputs()``; ``"auto"`` follows ``AUTO_FUSED``):
  ``cat_act_step`` (``include/cat_act.h``) straight from the env core's observation buffers -- per tick one ``torch.rand`` and ONE launch
  for all stacked policies; the recurrent state is updated in place;
* unfused (``False``; the CPU / fp32 path, other ray counts, the non-recurrent pair): the ``StackedNet`` chain and ``mappo._sample``,
  operation for operation what ``self_play.evaluate_agents`` does with a trainer -- from the same global generator state the actions are
  bit-identical to it.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import _learn_native, packing
from .mappo import MAPPOTrainer, _sample
from .stacked import HIDDEN, StackedNet, _module_for, _net_shapes, load_agent_state_dict

META_KEY = MAPPOTrainer.META_KEY
# What ``fused="auto"`` resolves to where the kernel applies.  No timing of ``cat_act_step`` against the chain has been recorded yet
# (``tools/act_bench.py`` takes it; profiles/act_step.txt holds the accuracy run only), so "auto" stays on the measured path, the chain;
# ``fused=True`` asks for the kernel (an error where it does not apply), ``fused="kernel"`` takes it where it applies and the chain elsewhere
# (what the explicit opt-ins ``watch --fused-act`` and ``self_play --fused-eval`` pass).
AUTO_FUSED = False


class PolicyParams:
    """The policy blocks of G agents as rows of one ``[G, P]`` buffer in the compute dtype, with the surface of ``stacked.FlatParams`` that
    ``StackedNet`` and ``load_agent_state_dict`` use: no fp32 master copy, no gradient buffer."""

    def __init__(self, R: int, G: int, device, compute_dtype: torch.dtype, arch: str = "lstm"):
        shapes = {f"policy.{n}": s for n, s in _net_shapes("policy", R, arch).items()}
        self.G, self.names, self.compute_dtype = G, list(shapes), compute_dtype
        self.offsets, off = {}, 0
        for n, shp in shapes.items():
            k = int(math.prod(shp))
            self.offsets[n] = (off, k, tuple(shp))
            off += (k + 7) // 8 * 8                                              # 16-byte aligned starts in bf16, as FlatParams
        self.P = off
        self.lp = torch.zeros(G, self.P, dtype=compute_dtype, device=device)
        self.master = self.lp                                                    # loaders write here; rounding = FlatParams.refresh's
        self.views = {n: self.lp[:, o:o + k].view(G, *shp) for n, (o, k, shp) in self.offsets.items()}

    def master_view(self, name: str) -> torch.Tensor:
        return self.views[name]

    def refresh(self) -> None:
        pass


class _Group:
    """The agents evaluated as one stacked policy: what the act tick reads of a ``mappo.RoleLearner``."""

    def __init__(self, key: str, agents: List[str], indices: List[int], policy: StackedNet, device):
        self.role, self.agents, self.indices, self.policy, self.fp = key, agents, indices, policy, policy.fp
        self.agent_roles = [a.split("_")[0] for a in agents]
        self.G = len(agents)
        self.index_t = torch.tensor(indices, dtype=torch.long, device=device)


def _load_file(source) -> dict:
    sd = torch.load(source, map_location="cpu", weights_only=True) if isinstance(source, (str, Path)) else source
    if sd.get("format") == "cat-mappo-2":                                        # round-2 files, as MAPPOTrainer.load_state_dict
        sd = {a: sd["models"][a] for a in sd["models"]}
    return sd


class PolicyActor:
    def __init__(self, groups: Sequence, agents: List[str], num_envs: int, num_rays: int, device, normalize_inputs: bool = False,
                 fused: Union[str, bool] = "auto", row_tile: int = 0):
        self.groups = {g.role: g for g in groups}
        self.agents, self.N, self.R, self.device = list(agents), num_envs, num_rays, torch.device(device)
        self.normalize_inputs = normalize_inputs
        self.row_tile = row_tile
        d, t = 1.0 / 400.0, 0.25                       # ray length, number of type codes - 1 (MAPPOTrainer's scales)
        self._pin_scale = torch.tensor([d] * num_rays + [t] * num_rays, device=self.device)
        self._scales = (d, t) if normalize_inputs else (1.0, 1.0)
        self.actions = torch.zeros(num_envs, len(self.agents), dtype=torch.int32, device=self.device)
        self.state = {k: g.policy.initial_state(num_envs) for k, g in self.groups.items()}
        can = self.fusable()
        if fused is True and not can:
            raise ValueError("fused=True needs a GPU, bf16 parameters, the recurrent policies and 64 or 90 rays (include/cat_act.h)")
        assert fused in (True, False, "auto", "kernel"), fused
        self.fused = bool(can and (fused is True or fused == "kernel" or (fused == "auto" and AUTO_FUSED)))
        self._keep = torch.zeros(num_envs, dtype=torch.float32, device=self.device) if self.fused else None
        self._params = {}                              # group -> the kernel's parameter block (pointers into the views: built once)

    # ------------------------------------------------------------------ construction
    def fusable(self) -> bool:
        if self.device.type != "cuda":
            return False
        A = len(self.agents)
        return all(g.policy.arch == "lstm" and g.fp.compute_dtype == torch.bfloat16 and _learn_native.act_supported(g.G, self.N, A, self.R)
                   for g in self.groups.values())

    @classmethod
    def from_trainer(cls, runner: MAPPOTrainer, fused: Union[str, bool] = "auto", row_tile: int = 0) -> "PolicyActor":
        """An actor over the trainer's own policy parameters (no copy: an update of the trainer is seen by the actor)."""
        return cls(list(runner.roles.values()), runner.agents, runner.N, runner.R, runner.device, runner.tcfg.normalize_inputs, fused, row_tile)

    @classmethod
    def from_checkpoint(cls, source, env, roles: Optional[Sequence[str]] = None, fused: Union[str, bool] = "auto", compute_bf16: bool = True,
                        normalize_inputs: bool = False, recurrent: bool = True, seed: int = 0, device=None, row_tile: int = 0) -> "PolicyActor":
        """``source``: a checkpoint file (or its loaded dict) in either layout ``MAPPOTrainer.load_state_dict`` reads -- this project's
        (``__cat__``) or the reference's / skrl's (``{agent: {"policy": ..., "value": ..., "optimizer": ...}}``) -- or ``{role: source}`` to
        take the cops from one and the thieves from another, or None.  Only the POLICY blocks are copied to the device.  ``roles``: load
        these roles only.  Agents that no source covers keep the initial weights a trainer seeded with ``seed`` would give them."""
        device = torch.device(device) if device is not None else getattr(env, "device", torch.device("cpu"))
        agents = list(env.possible_agents)
        R = env.observation_spaces[agents[0]]["distance"].shape[0]
        dt = torch.bfloat16 if (compute_bf16 and device.type == "cuda") else torch.float32
        arch = "lstm" if recurrent else "mlp"
        fp = PolicyParams(R, len(agents), device, dt, arch)
        with torch.no_grad():
            for g in range(len(agents)):               # init_from_modules' policy half: the policy is the first module constructed
                gen_state = torch.random.get_rng_state()
                torch.manual_seed(seed * 1000 + g)
                for n, v in _module_for("policy", R, arch).state_dict().items():
                    fp.views[f"policy.{n}"][g].copy_(v)
                torch.random.set_rng_state(gen_state)
        key = "+".join(r for r in ("cop", "thief") if any(a.startswith(r) for a in agents))
        actor = cls([_Group(key, agents, list(range(len(agents))), StackedNet("policy", R, fp, arch), device)], agents, env.num_envs, R, device,
                    normalize_inputs, fused, row_tile)
        if source is not None:
            actor.load(source, roles)
        return actor

    @torch.no_grad()
    def load(self, source, roles: Optional[Sequence[str]] = None) -> None:
        """Copy the policy blocks of ``source`` (see ``from_checkpoint``) into this actor's parameters; ``roles`` restricts a single
        source to these roles.  (An actor made by ``from_trainer`` shares the trainer's buffers: load into the trainer instead.)"""
        if isinstance(source, dict) and source and all(k in ("cop", "thief") for k in source):
            for role, src in source.items():
                if roles is None or role in roles:
                    self.load(src, [role])
            return
        sd = _load_file(source)
        for grp in self.groups.values():
            assert isinstance(grp.fp, PolicyParams), "this actor shares a trainer's parameters"
            for g, a in enumerate(grp.agents):
                if roles is not None and a.split("_")[0] not in roles:
                    continue
                if a not in sd:
                    raise KeyError(f"checkpoint holds no agent {a!r} (it has {sorted(k for k in sd if k != META_KEY)})")
                load_agent_state_dict(grp.fp, g, sd[a], kinds=("policy",))

    # ------------------------------------------------------------------ footprint
    @property
    def parameter_bytes(self) -> int:
        """Bytes of the policy blocks this actor reads (the compute-dtype copy; alignment padding not counted)."""
        return sum(g.G * k * g.fp.views[n].element_size() for g in self.groups.values()
                   for n, (_, k, _) in g.fp.offsets.items() if n.startswith("policy."))

    @property
    def state_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for st in self.state.values() for t in st)

    # ------------------------------------------------------------------ recurrent state
    @torch.no_grad()
    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zero the recurrent state of every slot, or of the slots where ``mask`` (bool [N]) is set."""
        for st in self.state.values():
            for t in st:
                if mask is None:
                    t.zero_()
                else:
                    t.masked_fill_(mask.view(1, 1, -1, 1), 0)

    def get_state(self, out=None):
        """A copy of the recurrent state (into ``out``, a previous result, when given): ``set_state`` puts it back."""
        if out is None:
            return {k: tuple(t.clone() for t in st) for k, st in self.state.items()}
        for k, st in self.state.items():
            for dst, src in zip(out[k], st):
                dst.copy_(src)
        return out

    def set_state(self, state) -> None:
        for k, st in self.state.items():
            for dst, src in zip(st, state[k]):
                dst.copy_(src)

    # ------------------------------------------------------------------ the act tick
    @torch.no_grad()
    def act(self, env, starts: Optional[torch.Tensor] = None, greedy: bool = False, random_roles: Tuple[str, ...] = (), obs=None,
            logits_out=None, logp_out=None) -> torch.Tensor:
        """Every agent's action for the env's current observations -> ``self.actions`` [N, A] int32 (returned).  ``starts`` (bool [N]): an
        episode starts in these slots, their state is taken as zero; None carries every state.  ``greedy``: the largest logit (lowest
        index on ties) instead of a draw.  ``random_roles``: these roles act uniformly at random.  ``obs``: the observation dictionaries
        the env's last ``step`` / ``reset`` returned (unfused path; fetched from the env when omitted).  ``logits_out`` / ``logp_out``
        (fused path, one group): the kernel's optional outputs."""
        if self.fused:
            raw = env.raw_outputs()
            keep = None
            if starts is not None:
                keep = torch.logical_not(starts, out=self._keep)
            for k, g in self.groups.items():
                if k not in self._params:
                    self._params[k] = _learn_native.act_params({n: g.policy.w(n) for n in _learn_native.ACT_PARAM_NAMES})
                mask = sum(1 << i for i, r in enumerate(g.agent_roles) if r in random_roles)
                h, c = self.state[k]
                u = torch.rand(g.G, self.N, device=self.device)
                _learn_native.act_step(raw, g.indices, self._params[k], h[0], c[0], keep, u, self.actions, self._scales[0], self._scales[1],
                                       greedy, mask, logits_out, logp_out, self.row_tile)
            return self.actions
        if obs is None:
            obs = env.observations() if hasattr(env, "observations") else env._obs()
        N = self.N
        keep = None if starts is None else (~starts).view(1, N)
        for k, g in self.groups.items():               # self_play.evaluate_agents' action selection, operation for operation
            pin = torch.stack([packing.pack_policy_input(obs[a]) for a in g.agents])
            if self.normalize_inputs:
                pin = pin * self._pin_scale
            logits, self.state[k] = g.policy.forward(pin.unsqueeze(1), self.state[k], keep)
            if greedy:
                act = first_max_index(logits[:, 0].float())
            else:
                act = _sample(torch.log_softmax(logits[:, 0].float(), dim=-1))
            rnd = [ar in random_roles for ar in g.agent_roles]
            if any(rnd):
                rows = torch.tensor(rnd, device=self.device).view(g.G, 1)
                act = torch.where(rows, torch.randint(0, 4, (g.G, N), device=self.device), act)
            self.actions.index_copy_(1, g.index_t, act.t().to(torch.int32))
        return self.actions


def first_max_index(z: torch.Tensor) -> torch.Tensor:
    """The lowest index of the largest entry along the last axis."""
    k = z.shape[-1]
    idx = torch.arange(k, device=z.device).expand_as(z)
    return torch.where(z == z.max(dim=-1, keepdim=True).values, idx, torch.full_like(idx, k)).min(dim=-1).values
