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
from .scripted import SCRIPTS, ScriptedParams, scripted_step, target_of
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
                 fused: Union[str, bool] = "auto", row_tile: int = 0, env_agents: Optional[List[str]] = None):
        self.groups = {g.role: g for g in groups}
        self.agents, self.N, self.R, self.device = list(agents), num_envs, num_rays, torch.device(device)
        self.env_agents = list(agents) if env_agents is None else list(env_agents)     # the columns of the env's action matrix
        self.normalize_inputs = normalize_inputs
        self.row_tile = row_tile
        d, t = 1.0 / 400.0, 0.25                       # ray length, number of type codes - 1 (MAPPOTrainer's scales)
        self._pin_scale = torch.tensor([d] * num_rays + [t] * num_rays, device=self.device)
        self._scales = (d, t) if normalize_inputs else (1.0, 1.0)
        self.actions = torch.zeros(num_envs, len(self.env_agents), dtype=torch.int32, device=self.device)
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
        A = len(self.env_agents)
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


class LeagueActor(PolicyActor):
    """A ``PolicyActor`` whose env slots are cut into contiguous SEGMENTS, each naming per agent which parameter set of a BANK plays there
    (or that the agent acts uniformly at random): one act tick plays many match-ups at once -- every archived opponent of an evaluation, or
    a block of cells of a cross-play table.

        actor = LeagueActor.from_env(env, sets=4)
        actor.load_set(0, "cops/cop_iter_3.pt", "cop_0") ...
        actor.set_matchups([(0, 8, {"cop_0": 0, "cop_1": 0, "thief_0": 2}), (8, 16, {"cop_0": 1, "cop_1": 1, "thief_0": "random"})])
        actions = actor.act(env, starts)

    An agent may also follow a script of ``selfplay.scripted`` in a segment (``"chase"`` / ``"evade"``): fused, the league kernel is told
    "random" for it and a second launch, ``cat_rollout_scripted`` with the same uniform numbers and segment bounds, writes its action
    column there; unfused, it draws its own ``torch.rand(stop - start)`` after the segment's other draws.  Match-ups without a scripted
    name run exactly the single launch / the generator sequence described below.

    fused: per tick one ``torch.rand(G, N)`` -- the draw a ``PolicyActor`` makes -- and ONE ``cat_act_league_step`` (include/cat_act.h).
    unfused: per segment the ``StackedNet`` chain over the G parameter rows the segment names, on that segment's rows of the inputs and of
    the state, then ``first_max_index`` / ``mappo._sample``; "random" draws ``torch.randint(0, 4, ...)`` and leaves its state rows alone."""

    def __init__(self, group: _Group, bank: PolicyParams, agents: List[str], num_envs: int, num_rays: int, device, normalize_inputs: bool = False,
                 fused: Union[str, bool] = "auto", row_tile: int = 0, env_agents: Optional[List[str]] = None):
        super().__init__([group], agents, num_envs, num_rays, device, normalize_inputs, fused, row_tile, env_agents)
        self.group, self.bank, self.sets = group, bank, bank.G
        self.table = None                              # _learn_native.LeagueTable of the current match-ups
        self._bank_params = None
        self._nets = {}                                # unfused: (set index per agent) -> StackedNet over a copy of those bank rows
        self.script_params = ScriptedParams()
        self.script_table = None                       # _learn_native.ScriptedTable while a segment names a script, else None
        self.script_state = None                       # int32 [G, N, 4] (scripted.py), allocated with the first scripted match-up
        self._targets = [target_of(a) for a in self.agents]

    @classmethod
    def from_env(cls, env, sets: int, fused: Union[str, bool] = "auto", compute_bf16: bool = True, normalize_inputs: bool = False,
                 recurrent: bool = True, seed: int = 0, device=None, row_tile: int = 0, agents: Optional[Sequence[str]] = None) -> "LeagueActor":
        """A bank of ``sets`` policy parameter rows for ``env``'s agents; set k starts from the weights ``torch.manual_seed(seed * 1000 + k)``
        gives a fresh policy module.  The other arguments as in ``PolicyActor.from_checkpoint``.
        ``agents``: a subset of ``env.possible_agents`` (in the env's order; for role training, one role's agents) -- the group, its
        recurrent state, ``set_matchups`` and the kernel's agent map then cover those agents only, and every other column of the action
        matrix is left alone on both paths.  None: all of them."""
        device = torch.device(device) if device is not None else getattr(env, "device", torch.device("cpu"))
        env_agents = list(env.possible_agents)
        if agents is None:
            agents = env_agents
        else:
            agents = list(agents)
            if not agents or len(set(agents)) != len(agents) or any(a not in env_agents for a in agents):
                raise ValueError(f"agents must be a non-empty subset of the env's agents {env_agents} without repeats: {agents}")
            agents = [a for a in env_agents if a in agents]
        R = env.observation_spaces[agents[0]]["distance"].shape[0]
        dt = torch.bfloat16 if (compute_bf16 and device.type == "cuda") else torch.float32
        arch = "lstm" if recurrent else "mlp"
        if sets < 1:
            raise ValueError("a bank needs at least one parameter set")
        bank = PolicyParams(R, sets, device, dt, arch)
        # the seeding below reaches every generator: the host's and this device's are put back (the actor's draws come from the latter)
        forked = [torch.cuda.current_device() if device.index is None else device.index] if device.type == "cuda" else []
        with torch.no_grad(), torch.random.fork_rng(devices=forked):
            for k in range(sets):
                torch.manual_seed(seed * 1000 + k)
                for n, v in _module_for("policy", R, arch).state_dict().items():
                    bank.views[f"policy.{n}"][k].copy_(v)
        key = "+".join(r for r in ("cop", "thief") if any(a.startswith(r) for a in agents))
        # the group's own G rows are scratch: what ``fusable`` / ``initial_state`` read of them is their shape, dtype and architecture
        grp = _Group(key, agents, [env_agents.index(a) for a in agents], StackedNet("policy", R, PolicyParams(R, len(agents), device, dt, arch), arch), device)
        return cls(grp, bank, agents, env.num_envs, R, device, normalize_inputs, fused, row_tile, env_agents)

    def load(self, source, roles=None) -> None:
        raise TypeError("a LeagueActor holds a bank of parameter sets: load_set(k, source, agent)")

    @torch.no_grad()
    def load_set(self, k: int, source, agent: str) -> None:
        """Copy the policy block of ``agent`` in ``source`` -- a checkpoint file or its loaded dict, in either layout ``PolicyActor.load``
        reads, or ``{agent: {"policy": state_dict}}`` -- into set ``k`` of the bank."""
        if not 0 <= k < self.sets:
            raise IndexError(f"set {k} of a bank of {self.sets}")
        sd = _load_file(source)
        if agent not in sd:
            raise KeyError(f"checkpoint holds no agent {agent!r} (it has {sorted(k_ for k_ in sd if k_ != META_KEY)})")
        load_agent_state_dict(self.bank, k, sd[agent], kinds=("policy",))
        self._nets.clear()

    def set_matchups(self, segments) -> None:
        """``segments``: [(start, stop, {agent: set index | "random" | "chase" | "evade"}), ...] -- contiguous row ranges that cover 0 .. N
        in order, at most ``_learn_native.ACT_MAX_SEGMENTS`` of them, every agent named in each.  The rules of ``cat_act_league_step``;
        ValueError otherwise."""
        segments = list(segments)
        if not segments:
            raise ValueError("no segments")
        bounds = [segments[0][0]]
        rows = [[] for _ in self.agents]
        scripts = [[] for _ in self.agents]
        for lo, hi, who in segments:
            if lo != bounds[-1]:
                raise ValueError(f"segment ({lo}, {hi}) does not begin where the one before it ends ({bounds[-1]})")
            bounds.append(hi)
            if set(who) != set(self.agents):
                raise ValueError(f"segment ({lo}, {hi}) must name exactly the agents {self.agents}: {sorted(who)}")
            for g, a in enumerate(self.agents):
                v = who[a]
                scripted = isinstance(v, str) and v in SCRIPTS
                if not (v == "random" or scripted or (isinstance(v, int) and not isinstance(v, bool) and v >= 0)):
                    raise ValueError(f"segment ({lo}, {hi}), {a}: {v!r} is neither a set index nor \"random\" nor one of {sorted(SCRIPTS)}")
                rows[g].append(-1 if v == "random" or scripted else v)
                scripts[g].append(SCRIPTS[v] if scripted else -1)
        table = _learn_native.league_table(self.N, len(self.agents), self.sets, bounds, rows)
        if any(v >= 0 for row in scripts for v in row):
            script_table = _learn_native.scripted_table(self.N, len(self.agents), bounds, scripts)
            if self.script_state is None:
                self.script_state = torch.zeros(len(self.agents), self.N, 4, dtype=torch.int32, device=self.device)
        else:
            script_table = None
        self.table, self.script_table = table, script_table

    @torch.no_grad()
    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        super().reset(mask)
        if self.script_state is not None:
            if mask is None:
                self.script_state.zero_()
            else:
                self.script_state.masked_fill_(mask.view(1, -1, 1), 0)

    def get_state(self, out=None):
        """``PolicyActor.get_state``, with the scripted agents' rows under ``"scripted"`` while there are any."""
        out = super().get_state(out)
        if self.script_state is not None:
            if "scripted" in out:
                out["scripted"].copy_(self.script_state)
            else:
                out["scripted"] = self.script_state.clone()
        return out

    def set_state(self, state) -> None:
        super().set_state(state)
        if self.script_state is not None and "scripted" in state:
            self.script_state.copy_(state["scripted"])

    @property
    def segments(self) -> List[Tuple[int, int]]:
        """[(start, stop)] of the current match-ups."""
        b = self.table.start
        return list(zip(b[:-1], b[1:]))

    @property
    def parameter_bytes(self) -> int:
        return sum(self.sets * k * self.bank.views[n].element_size() for n, (_, k, _) in self.bank.offsets.items())

    def _segment_net(self, sets: Tuple[int, ...]) -> StackedNet:
        """The stacked net whose row g holds bank set ``sets[g]`` (row 0's for a random agent: evaluated and thrown away)."""
        if sets not in self._nets:
            fp = PolicyParams(self.R, len(sets), self.device, self.bank.compute_dtype, self.group.policy.arch)
            fp.lp.copy_(self.bank.lp[[max(k, 0) for k in sets]])
            self._nets[sets] = StackedNet("policy", self.R, fp, self.group.policy.arch)
        return self._nets[sets]

    @torch.no_grad()
    def act(self, env, starts: Optional[torch.Tensor] = None, greedy: bool = False, random_roles: Tuple[str, ...] = (), obs=None,
            logits_out=None, logp_out=None, actions: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``PolicyActor.act`` under the current match-ups.  ``random_roles`` must stay empty: a random agent is "random" in its segments.
        ``logits_out`` [G, N, 4] is filled on both paths, ``logp_out`` [G, N] by the kernel only.
        ``actions`` (int32 [N, A] over ALL the env's agents, contiguous, on the actor's device): the actor writes its agents' columns there
        instead of into ``self.actions`` and returns it -- on the fused path it is the kernel's ``actions`` pointer (no copy); the columns
        of agents the actor does not cover are not touched."""
        if random_roles:
            raise ValueError("LeagueActor: name \"random\" in set_matchups instead of random_roles")
        if self.table is None:
            raise RuntimeError("LeagueActor.act before set_matchups")
        g, N = self.group, self.N
        if actions is None:
            actions = self.actions
        elif not (actions.dtype == torch.int32 and tuple(actions.shape) == tuple(self.actions.shape) and actions.is_contiguous()
                  and actions.device == self.actions.device):
            raise ValueError(f"actions must be a contiguous int32 {tuple(self.actions.shape)} tensor on {self.actions.device}")
        h, c = self.state[g.role]
        if self.fused:
            raw = env.raw_outputs()
            keep = None
            if starts is not None:
                keep = torch.logical_not(starts, out=self._keep)
            if self._bank_params is None:
                self._bank_params = _learn_native.act_params({n: self.bank.views[f"policy.{n}"] for n in _learn_native.ACT_PARAM_NAMES})
            u = torch.rand(g.G, N, device=self.device)
            _learn_native.act_league_step(raw, g.indices, self._bank_params, self.sets, self.table, None, h[0], c[0], keep, u, actions,
                                          self._scales[0], self._scales[1], greedy, logits_out, logp_out, self.row_tile)
            if self.script_table is not None:          # the scripted agents' columns in their segments, over the league kernel's "random"
                sp = self.script_params
                _learn_native.rollout_scripted(raw, g.indices, self._targets, self.script_table, u, keep, self.script_state, actions,
                                               sp.memory_ticks, sp.clear_min, sp.turn_prob)
            return actions
        if obs is None:
            obs = env.observations() if hasattr(env, "observations") else env._obs()
        pin = torch.stack([packing.pack_policy_input(obs[a]) for a in g.agents])
        if self.normalize_inputs:
            pin = pin * self._pin_scale
        for s, (lo, hi) in enumerate(self.segments):
            sets = tuple(row[s] for row in self.table.table)
            keep = None if starts is None else (~starts[lo:hi]).view(1, hi - lo)
            logits, (hn, cn) = self._segment_net(sets).forward(pin[:, lo:hi].unsqueeze(1), (h[:, :, lo:hi], c[:, :, lo:hi]), keep)
            if greedy:
                act = first_max_index(logits[:, 0].float())
            else:
                act = _sample(torch.log_softmax(logits[:, 0].float(), dim=-1))
            net = [i for i, k in enumerate(sets) if k >= 0]
            scripted = [] if self.script_table is None else [i for i, row in enumerate(self.script_table.rows) if row[s] >= 0]
            if len(net) + len(scripted) < g.G:
                rows = torch.tensor([k < 0 and i not in scripted for i, k in enumerate(sets)], device=self.device).view(g.G, 1)
                act = torch.where(rows, torch.randint(0, 4, (g.G, hi - lo), device=self.device), act)
            for i in scripted:                         # after the segment's other draws: one torch.rand(hi - lo) per scripted agent
                a = g.agents[i]
                st = self.script_state[i, lo:hi]
                a_s, new = scripted_step(obs[a]["distance"][lo:hi], obs[a]["object_type"][lo:hi], torch.rand(hi - lo, device=self.device), st,
                                         None if starts is None else ~starts[lo:hi], self.script_table.rows[i][s], self._targets[i],
                                         self.script_params)
                st.copy_(new)
                act[i] = a_s.to(act.dtype)
            if logits_out is not None:                 # [G, N, 4]: the rows of the agents that evaluated a network, as the kernel
                logits_out[net, lo:hi] = logits[net, 0].to(logits_out.dtype)
            if hn.shape[0]:                            # the recurrent pair: the rows of the agents that evaluated a network move
                h[:, net, lo:hi] = hn[:, net]
                c[:, net, lo:hi] = cn[:, net]
            actions[lo:hi].index_copy_(1, g.index_t, act.t().to(torch.int32))
        return actions


def first_max_index(z: torch.Tensor) -> torch.Tensor:
    """The lowest index of the largest entry along the last axis."""
    k = z.shape[-1]
    idx = torch.arange(k, device=z.device).expand_as(z)
    return torch.where(z == z.max(dim=-1, keepdim=True).values, idx, torch.full_like(idx, k)).min(dim=-1).values
