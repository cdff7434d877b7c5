#!/usr/bin/env python3
"""Self-play on the batched env: the reference's ``src/self_play_driver.py:83-117`` loop over
``training/orchestration.py:100-249`` (``_orchestrate_simultaneous_training_iteration``) and
``utils/agent_learning_utils.py:172-380`` (``train_simultaneously_and_evaluate`` / ``evaluate_agent``), with
``TrainingConfig`` of ``src/configs/training_config.py:3-12``.

Per iteration, as in the reference:

1. both roles continue from the latest checkpoint of their archive (model weights only -- the reference builds a
   fresh ``MAPPO`` and copies policy + value weights in, ``orchestration.py:121-211``; Adam starts fresh);
2. one ``trainer.train()``: all roles train simultaneously under the timestep schedule (``mappo.MAPPOTrainer.train``);
3. the newly trained cops are evaluated against up to 5 DISTINCT archived thief policies sampled by the configured
   strategy (PFSP), ``n_trial_episodes`` episodes each; per opponent ONE outcome -- "did the archived opponent win
   more episodes than the learner" -- is booked into that opponent's entry of the thief archive's ``win_rates.json``;
   then the same for the thieves against archived cops (``agent_learning_utils.py:233-380``);
4. the joint checkpoint ``joint_iter_{i}_full_agent.pt`` (every model, the optimiser state, the trainer position) is
   saved and copied into BOTH archives as ``{role}_iter_{i}.pt`` (``orchestration.py:225-245``).

Conscious deviation (quirk Q16): the reference's ``evaluate_agent`` loads each sampled opponent INTO the
agent it has just trained (``eval_agent = learned_agent`` is an alias, ``agent_learning_utils.py:253``), so the
checkpoint saved in step 4 holds the last sampled ARCHIVED policies of both roles instead of the trained ones.  Here
the opponents are loaded into a separate evaluation copy and the trained weights are what gets saved.

    python -m as_cops_and_thieves_amd.selfplay.self_play --map squarinth --envs 1024 --iterations 3 --timesteps 2000

**N GPUs of one node** (BASELINE configs[2]: 32768 envs sharded 8x, gradient all-reduce over xGMI):

    python -m as_cops_and_thieves_amd.selfplay.self_play --gpus 8 --map agh-map --envs 32768 ...

The command starts N fresh rank processes through ``torch.distributed.run`` as a CHILD process (never an exec; the parent has not
touched the GPU).  Rank r simulates the global env ids ``shard_envs(envs, r, N)`` (no data-path collective: SURVEY 8e), the ranks
open one RCCL group, and every optimiser step all-reduces ONE buffer -- the flat gradients | the KL statistics of all stacked
networks (``mappo.RoleLearner.minibatch_step``) -- so the replicas stay bit-identical and take the same early-stop decisions.
Rank 0 alone evaluates, writes checkpoints, archives and ``win_rates.json``; the others wait at a barrier and read the files.
"""
from __future__ import annotations

import argparse
import dataclasses
import inspect
import json
import os
import random
import sys
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

from ..environments import VecCopsEnv
from ..maps import load_preset
from . import archive
from .mappo import CFG_AGENT, MAPPOTrainer, RoleConfig, TrainerConfig, _sample


@dataclasses.dataclass
class TrainingConfig:
    """``src/configs/training_config.py:3-12``."""
    num_self_play_iterations: int = 40
    training_timesteps_per_role_training: int = 100_000
    archive_save_interval: int = 1
    policy_sample_strategy: str = "pfsp"
    win_rate_buffer_size: int = 20
    n_trial_episodes: int = 5
    cop_role_prefix: str = "cop"
    thief_role_prefix: str = "thief"
    num_opponents_to_evaluate: int = 5        # evaluate_agent(num_additional_opponents_to_evaluate=5)
    num_training_opponents: int = 8           # role training (train_role_league): archived opponents a phase trains against at once, 1..32


def _skip_kw(frame_skip: int) -> dict:
    """The keyword that makes ``env.step`` a frame-skip step; empty for 1, so that envs without the keyword keep working."""
    if isinstance(frame_skip, bool) or not isinstance(frame_skip, int) or frame_skip < 1:
        raise ValueError(f"frame_skip must be an integer >= 1, got {frame_skip!r}")
    return {} if frame_skip == 1 else {"repeat": frame_skip}


@torch.no_grad()
def evaluate_agents(env, runner: Optional[MAPPOTrainer], n_episodes: int, random_roles: Tuple[str, ...] = (), actor=None,
                    frame_skip: int = 1) -> Tuple[float, float]:
    """``src/utils/eval_pfsp_agents.py:7-59``: ``n_episodes`` episodes with every model frozen, actions sampled from
    the policies (skrl ``policy.act``), an episode ends at its first termination and is a win of ``infos["winner"]``.
    Returns (cop wins / n, thief wins / n).  The batched form plays the episodes in parallel, one per env slot
    (``env.num_envs >= n_episodes``; the first episode of the first ``n_episodes`` slots counts).  ``random_roles``:
    these roles act uniformly at random instead (a fixed yardstick opponent; not part of the reference protocol).
    ``actor`` (``actor.PolicyActor``): the policies act through it instead of through ``runner`` (which may then be None).
    ``frame_skip`` k > 1: the policies decide once per ``env.step(actions, repeat=k)``, i.e. every k env ticks of an episode."""
    N = env.num_envs
    who = actor if actor is not None else runner          # sizes, device and agent names: the actor's or the trainer's
    assert N >= n_episodes and N == who.N
    skip = _skip_kw(frame_skip)
    obs, _ = env.reset()
    starts = torch.ones(N, dtype=torch.bool, device=who.device)
    state = _initial_states(runner, actor, N)
    winner = torch.full((N,), -1, dtype=torch.int8, device=who.device)
    open_ = torch.ones(N, dtype=torch.bool, device=who.device)
    open_[n_episodes:] = False
    actions = torch.zeros(N, len(who.agents), dtype=torch.int32, device=who.device)
    for _ in range(env.max_step_count + 2):
        if actor is not None:
            actions = actor.act(env, starts, random_roles=random_roles, obs=obs)
        else:
            _trainer_actions(runner, obs, state, starts, actions, random_roles)
        obs, _, terms, _, infos = env.step(actions, **skip)
        done = terms[who.agents[0]]
        first = open_ & done
        winner = torch.where(first, infos["winner"].to(torch.int8), winner)
        open_ = open_ & ~done
        starts = done.clone()
        if not bool(open_.any()):                       # one host sync per tick, on the evaluation path only
            break
    w = winner[:n_episodes]
    return float((w == 0).sum()) / n_episodes, float((w == 1).sum()) / n_episodes


def _initial_states(runner, actor, N: int):
    """The recurrent states an evaluation loop carries for the trainer's policies; with an actor the actor carries its own (zeroed here)."""
    if actor is not None:
        actor.reset()
        return {}
    return {r: rl.policy.initial_state(N) for r, rl in runner.roles.items()}


def _trainer_actions(runner: MAPPOTrainer, obs, state, starts: torch.Tensor, actions: torch.Tensor, random_roles: Tuple[str, ...]) -> None:
    """One tick's action selection through the trainer's stacked policies, into ``actions`` [N, A]: sampled from the policies (skrl
    ``policy.act``), ``random_roles`` uniformly at random; ``state`` (role -> recurrent state) is advanced in place."""
    N = runner.N
    keep = (~starts).view(1, N)
    for r, rl in runner.roles.items():
        pin = torch.stack([runner_pack(obs[a]) for a in rl.agents])
        if runner.tcfg.normalize_inputs:
            pin = pin * runner._pin_scale
        logits, state[r] = rl.policy.forward(pin.unsqueeze(1), state[r], keep)
        act = _sample(torch.log_softmax(logits[:, 0].float(), dim=-1))
        rnd = [ar in random_roles for ar in rl.agent_roles]
        if any(rnd):                                # a uniformly random opponent (not part of the reference protocol)
            rows = torch.tensor(rnd, device=runner.device).view(rl.G, 1)
            act = torch.where(rows, torch.randint(0, 4, (rl.G, N), device=runner.device), act)
        actions.index_copy_(1, rl.index_t, act.t().to(torch.int32))


class _Rewind:
    """What a later evaluation on the same env can see of this one, kept per tick for the ticks since the last poll: the global
    generators ``_sample`` / ``torch.randint`` draw from (host-side reads) and a device-side copy of the env's state
    (``get_env_state``: no synchronisation; the copies of a tick ``window`` ticks back are overwritten in place).  ``restore(tick)`` puts
    both back to where they stood after that tick."""

    def __init__(self, env, device, window: int, actor=None):
        self.env, self.device, self.window, self.kept, self.actor = env, device, window, {}, actor

    def keep(self, tick: int) -> None:
        old = self.kept.get(tick % self.window)
        rng = (torch.get_rng_state(), torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None)
        held = None if self.actor is None else self.actor.get_state(out=None if old is None else old[3])   # the actor's h / c after this tick
        self.kept[tick % self.window] = (tick, rng, self.env.get_env_state(out=None if old is None else old[2]), held)

    def restore(self, tick: int) -> None:
        kept_tick, rng, state, held = self.kept[tick % self.window]
        assert kept_tick == tick, (kept_tick, tick)
        self.env.set_env_state(**state)
        if held is not None:
            self.actor.set_state(held)
        torch.set_rng_state(rng[0])
        if rng[1] is not None:
            torch.cuda.set_rng_state(rng[1], self.device)


@torch.no_grad()
def evaluate_agents_tracked(env, runner: Optional[MAPPOTrainer], n_episodes: int, random_roles: Tuple[str, ...] = (),
                            poll_every: int = 32, actor=None, frame_skip: int = 1) -> Tuple[float, float]:
    """``evaluate_agents`` with the book-keeping done on the device by the env's ``episode_tracker`` (``episodes.EpisodeTracker``,
    which the env feeds on every ``step``): the same tick loop, but the host looks at the number of slots still owing an episode only
    every ``poll_every`` ticks instead of every tick, and a slot plays several episodes in a row, so any ``n_episodes`` is allowed.
    Slot n counts its first ``n_episodes // N + (n < n_episodes % N)`` episodes.  For ``n_episodes <= N`` that is the first episode of
    the first ``n_episodes`` slots: from the same generator state the result equals ``evaluate_agents``'s exactly -- the ticks played
    between the last counted episode and the next poll count nothing.  Those ticks are then taken back (``_Rewind``): the global
    generators and the env's state are put back to where the tick that ended the last counted episode left them, which is where
    ``evaluate_agents`` stops, so a later evaluation on the same env starts from the same state either way.  Beyond the surface
    ``evaluate_agents`` uses, the env must offer ``episode_tracker`` and ``get_env_state(out=None)`` / ``set_env_state(**state)``.
    Cost of ``poll_every``: the window holds that many full copies of the env state on the device (a few hundred bytes per slot
    each), and every tick makes one state-copy launch and two host reads of generator state (a new 5 KB CPU snapshot each).
    ``actor``: as in ``evaluate_agents``; its recurrent state is kept and put back with the env's.
    ``frame_skip`` k > 1: one decision per ``env.step(actions, repeat=k)``; ``poll_every`` and the rewind then count decisions, the tracker
    still counts lengths in env ticks (the env hands it every row's tick count), and the decision that closed the last counted episode
    is kept on the device, since the slots' tick counts no longer tell it."""
    N = env.num_envs
    who = actor if actor is not None else runner          # sizes, device and agent names: the actor's or the trainer's
    assert N == who.N and n_episodes >= 1 and poll_every >= 1
    skip = _skip_kw(frame_skip)
    tracker = env.episode_tracker
    obs, _ = env.reset()
    quota = torch.full((N,), n_episodes // N, dtype=torch.int32)
    quota[:n_episodes % N] += 1
    tracker.set_quota(quota)
    tracker.abandon()
    tracker.clear()
    starts = torch.ones(N, dtype=torch.bool, device=who.device)
    state = _initial_states(runner, actor, N)
    actions = torch.zeros(N, len(who.agents), dtype=torch.int32, device=who.device)
    limit = int(quota.max()) * env.max_step_count + 2
    rewind = _Rewind(env, who.device, poll_every, actor)
    stats, tick = None, 0
    if skip:    # the decision after which the last slot filled its quota, found without a synchronisation
        slots = tracker.per_slot()
        owing = slots["finished"] < slots["quota"]
        last_close = torch.zeros((), dtype=torch.int64, device=who.device)
    while tick < limit:
        if actor is not None:
            actions = actor.act(env, starts, random_roles=random_roles, obs=obs)
        else:
            _trainer_actions(runner, obs, state, starts, actions, random_roles)
        obs, _, terms, _, _ = env.step(actions, **skip)
        starts = terms[who.agents[0]].clone()
        tick += 1
        rewind.keep(tick)
        if skip:
            still = slots["finished"] < slots["quota"]
            last_close = torch.where((owing & ~still).any(), torch.full_like(last_close, tick), last_close)
            owing = still
        if tick % poll_every == 0 or tick == limit:
            stats = tracker.summary()                   # the one host synchronisation of these poll_every ticks
            if stats["open_slots"] == 0:
                break
    assert stats is not None and stats["open_slots"] == 0 and stats["episodes"] == n_episodes, stats
    # a slot's counted episodes are its first ones after the reset, back to back: the last of them ended at tick max(len_sum), which
    # lies after the poll before this one (slots were still open then), i.e. within the poll_every ticks kept
    rewind.restore(int(last_close) if skip else int(tracker.per_slot()["len_sum"].max()))
    return float(stats["cop_wins"]) / n_episodes, float(stats["thief_wins"]) / n_episodes


@torch.no_grad()
def mean_reward_per_tick(env, runner: Optional[MAPPOTrainer], ticks: int, random_roles: Tuple[str, ...] = (), actor=None) -> Dict[str, float]:
    """Diagnostic (not part of the reference protocol): reset ``env``, act for ``ticks`` ticks with sampled actions
    (``random_roles`` uniformly at random) and return every agent's mean reward per tick -- the quantity PPO maximises,
    measured from the same starting conditions whenever it is called.  ``actor``: as in ``evaluate_agents``."""
    N = env.num_envs
    who = actor if actor is not None else runner          # sizes, device and agent names: the actor's or the trainer's
    assert N == who.N
    obs, _ = env.reset()
    starts = torch.ones(N, dtype=torch.bool, device=who.device)
    state = _initial_states(runner, actor, N)
    actions = torch.zeros(N, len(who.agents), dtype=torch.int32, device=who.device)
    total = {a: torch.zeros((), device=who.device) for a in who.agents}
    for _ in range(ticks):
        if actor is not None:
            actions = actor.act(env, starts, random_roles=random_roles, obs=obs)
        else:
            _trainer_actions(runner, obs, state, starts, actions, random_roles)
        obs, rewards, terms, _, _ = env.step(actions)
        for a in who.agents:
            total[a] += rewards[a].float().mean()
        starts = terms[who.agents[0]].clone()
    return {a: float(v) / ticks for a, v in total.items()}


def runner_pack(obs_agent):
    from .. import packing
    return packing.pack_policy_input(obs_agent)


def _draw_new_opponent(opponent_archive: Path, opponent_role: str, tc: TrainingConfig, rng: random.Random, seen) -> Optional[str]:
    """One archived ``opponent_role`` policy whose file name is not in ``seen``: 20 tries by the configured strategy, then 20 uniformly
    (``agent_learning_utils.py:262-300``); None when none turned up."""
    for strategy in (tc.policy_sample_strategy, "random"):
        for _ in range(20):
            cand = archive.sample_policy_from_archive(opponent_archive, opponent_role, strategy, rng=rng)
            if cand is None:
                break
            if Path(cand).name not in seen:
                return cand
    return None


def evaluate_agent(eval_env, evaluator: MAPPOTrainer, learned: MAPPOTrainer, learned_role: str, opponent_role: str,
                   opponent_archive: Path, tc: TrainingConfig, rng: random.Random, log=print, tracked: bool = False,
                   fused_eval: bool = False, frame_skip: int = 1) -> Dict[str, bool]:
    """``agent_learning_utils.py:233-380``: the newly trained ``learned_role`` against up to
    ``tc.num_opponents_to_evaluate`` distinct archived ``opponent_role`` policies.  Returns {opponent file: opponent won}.
    ``tracked``: play the episodes through ``evaluate_agents_tracked`` (``eval_env`` must feed an ``episode_tracker``).
    ``fused_eval``: ``evaluator`` is a ``PolicyActor`` (``from_checkpoint(None, eval_env, ...)``) and the episodes are played through it.
    ``frame_skip``: env ticks per decision of the episodes played (``evaluate_agents``)."""
    results: Dict[str, bool] = {}
    if fused_eval:
        evaluator.load({a: learned.agent_models(a) for a in learned.agents}, roles=[learned_role])
    else:
        evaluator.load_state_dict(learned.state_dict(), roles=[learned_role], optimizer=False)
    seen = set()
    for i in range(tc.num_opponents_to_evaluate):
        path = _draw_new_opponent(opponent_archive, opponent_role, tc, rng, seen)
        if path is None:
            log(f"[self-play] no new distinct {opponent_role} opponent for evaluation round {i + 1}/{tc.num_opponents_to_evaluate}")
            break
        name = Path(path).name
        seen.add(name)
        if fused_eval:
            evaluator.load(path, roles=[opponent_role])                  # the policy blocks only
        else:
            evaluator.load_state_dict(torch.load(path, map_location=evaluator.device, weights_only=True), roles=[opponent_role],
                                      optimizer=False)                   # copy_role_models: policy + value weights
        play = evaluate_agents_tracked if tracked else evaluate_agents
        cop_rate, thief_rate = (play(eval_env, None, tc.n_trial_episodes, actor=evaluator, frame_skip=frame_skip) if fused_eval
                                else play(eval_env, evaluator, tc.n_trial_episodes, frame_skip=frame_skip))
        opponent_won = (thief_rate > cop_rate) if learned_role == tc.cop_role_prefix else (cop_rate > thief_rate)
        archive.update_policy_win_rate(opponent_archive, name, opponent_won, tc.win_rate_buffer_size)
        results[name] = opponent_won
        log(f"[self-play]   {learned_role} vs {name}: cop {cop_rate:.2f} thief {thief_rate:.2f} -> opponent {'won' if opponent_won else 'lost'}")
    return results


@torch.no_grad()
def evaluate_league(env, actor, episodes_per_segment=None, frame_skip: int = 1, positions: bool = False, greedy: bool = False) -> Dict[str, object]:
    """``evaluate_agents``' loop -- the first episode of every slot, one poll per tick -- under the match-ups of a ``LeagueActor``: all its
    segments play at once.  ``episodes_per_segment``: an int or one int per segment -- only the first that many slots of a segment count
    (None: all of them; 0 for a segment that merely fills the env).  Returns per segment (lists in segment order) ``cop_wins`` (winner 0),
    ``thief_wins`` (winner 1 before the step limit), ``timeouts`` (the step limit ran out; not the cops' win) -- the three add up to the
    segment's counted slots -- and ``episodes``; per slot ``winner`` (int8, -1 where nothing counted) and ``length`` (ticks of the counted
    episode, int32); and ``ticks``, the steps of the loop played.  ``frame_skip`` k > 1: one decision per ``env.step(actions, repeat=k)``;
    ``length`` stays in env ticks (the sum of the slot's ``infos["ticks"]``), ``ticks`` counts decisions.
    ``positions``: the env's ``position_tracker`` (``VecCopsEnv(track_positions=CELL, position_groups >= segments)``) is cleared and set up
    like the accounting here -- one group per segment, a quota of the first episode of every counted slot, none of the others -- so that
    afterwards it holds the maps of exactly the counted episodes; ``out["positions"]`` is its ``summary()``.
    ``greedy``: the networks take their largest logit instead of a draw (``LeagueActor.act(greedy=True)``)."""
    N = env.num_envs
    assert N == actor.N and actor.table is not None
    tracker = env.position_tracker if positions else None      # (an env without one raises here, before anything is played)
    skip = _skip_kw(frame_skip)
    segments = actor.segments
    quota = episodes_per_segment
    if quota is None or isinstance(quota, int):
        quota = [quota] * len(segments)
    assert len(quota) == len(segments)
    dev = actor.device
    open_ = torch.ones(N, dtype=torch.bool, device=dev)
    for (lo, hi), q in zip(segments, quota):
        if q is not None:
            assert 0 <= q <= hi - lo, (lo, hi, q)
            open_[lo + q:hi] = False
    counted = open_.clone()
    if tracker is not None:
        tracker.clear()
        tracker.set_groups(bounds=[0] + [hi for _, hi in segments])
        tracker.set_quota(open_.to(torch.int32))
    obs, _ = env.reset()
    actor.reset()
    starts = torch.ones(N, dtype=torch.bool, device=dev)
    winner = torch.full((N,), -1, dtype=torch.int8, device=dev)
    timeout = torch.zeros(N, dtype=torch.bool, device=dev)
    length = torch.zeros(N, dtype=torch.int32, device=dev)
    played = torch.zeros(N, dtype=torch.int32, device=dev)      # frame_skip > 1: env ticks of the slot so far
    ticks = 0
    for _ in range(env.max_step_count + 2):
        if not bool(counted.any()):
            break
        actions = actor.act(env, starts, obs=obs, **({"greedy": True} if greedy else {}))
        obs, _, terms, truncs, infos = env.step(actions, **skip)
        ticks += 1
        done = terms[actor.agents[0]]
        first = open_ & done
        winner = torch.where(first, infos["winner"].to(torch.int8), winner)
        timeout = torch.where(first, truncs[actor.agents[0]], timeout)
        if skip:
            played = played + infos["ticks"]
        length = torch.where(first, played if skip else torch.full_like(length, ticks), length)
        open_ = open_ & ~done
        starts = done.clone()
        if not bool(open_.any()):                       # one host sync per tick, as evaluate_agents
            break
    w, t = winner.cpu(), timeout.cpu()
    out = {"cop_wins": [], "thief_wins": [], "timeouts": [], "episodes": [], "winner": winner, "length": length, "ticks": ticks}
    for (lo, hi), q in zip(segments, quota):
        hi = hi if q is None else lo + q
        out["cop_wins"].append(int((w[lo:hi] == 0).sum()))
        out["thief_wins"].append(int(((w[lo:hi] == 1) & ~t[lo:hi]).sum()))
        out["timeouts"].append(int(((w[lo:hi] != 0) & t[lo:hi]).sum()))
        out["episodes"].append(hi - lo)
    if tracker is not None:
        out["positions"] = tracker.summary()
    return out


@torch.no_grad()
def evaluate_by_separation(env, actor, bands, episodes: int, source=None, who=None, frame_skip: int = 1, greedy: bool = False, field=None) -> Dict[str, object]:
    """The cops' win rate as a function of the INITIAL geodesic separation -- what a checkpoint has learned, "catches from 6 hops, not from
    30", where one win rate says nothing.  The env's slots are cut into ``len(bands)`` contiguous segments of ``episodes`` slots
    (``env.num_envs == len(bands) * episodes``); segment s takes ``bands[s] = (lo, hi)`` through a ``GeodesicSpawner`` attached for the
    duration (``set_band(lo, hi, slots=)``), so the first episode of every slot starts with each cop lo .. hi hops from a thief; then ONE
    ``evaluate_league`` pass.  ``actor``: a ``LeagueActor`` over ``env``.  ``source`` (a ``MAPPOTrainer`` or a checkpoint, as in
    ``evaluate_against_scripts``) is loaded into sets 0 .. A - 1 and plays every agent; or ``who`` ({agent: set index | "random" |
    "chase" | "evade"}) names the players of sets loaded beforehand; with neither, the actor's own match-ups must already be these
    segments.  ``field``: an arena ``NavField`` of the env to share.
    Returns {"bands", "episodes", "cop_wins", "thief_wins", "timeouts" (of the first episode of every slot, lists in band order),
    "cop_win_rate", "fallback_share" (per band the share of slots the rule could not place: they started from the map's own spawn),
    "ticks"}.  The env's spawner is detached again afterwards, whatever happens."""
    from .curriculum import GeodesicSpawner, check_band
    bands = [check_band(int(lo), int(hi)) for lo, hi in bands]
    S = len(bands)
    if S < 1 or episodes < 1 or env.num_envs != S * episodes:
        raise ValueError(f"evaluate_by_separation plays {S} bands of {episodes} episodes: the env must have {S * episodes} slots, not {env.num_envs}")
    agents = list(env.possible_agents)
    if source is not None:
        if actor.sets < len(agents) or list(actor.agents) != agents:
            raise ValueError(f"the actor must cover {agents} with at least {len(agents)} sets")
        for g, a in enumerate(agents):
            actor.load_set(g, {a: source.agent_models(a)} if isinstance(source, MAPPOTrainer) else source, a)
        who = {a: g for g, a in enumerate(agents)}
    bounds = [(s * episodes, (s + 1) * episodes) for s in range(S)]
    if who is not None:
        actor.set_matchups([(lo, hi, dict(who)) for lo, hi in bounds])
    elif [tuple(b) for b in actor.segments] != bounds:
        raise ValueError(f"without source or who the actor's match-ups must be the {S} segments {bounds}, not {list(actor.segments)}")
    spawner = GeodesicSpawner(env, *bands[0], field=field)
    for (lo, hi), (b0, b1) in zip(bands, bounds):
        spawner.set_band(lo, hi, slots=slice(b0, b1))
    env.set_spawner(spawner)
    try:
        res = evaluate_league(env, actor, frame_skip=frame_skip, greedy=greedy)
    finally:
        env.set_spawner(None)
    placed = spawner.reset_placed.cpu().view(S, episodes).float()
    return {"bands": [list(b) for b in bands], "episodes": res["episodes"], "cop_wins": res["cop_wins"], "thief_wins": res["thief_wins"],
            "timeouts": res["timeouts"], "cop_win_rate": [c / episodes for c in res["cop_wins"]],
            "fallback_share": [float(1.0 - p.mean()) for p in placed], "ticks": res["ticks"]}


BASELINE_SEGMENTS = ("cops_vs_evade", "cops_vs_random", "chase_vs_thieves", "random_vs_thieves")


def evaluate_against_scripts(eval_env, source, episodes: int, greedy: bool = False, frame_skip: int = 1, fused="kernel", actor=None) -> Dict[str, object]:
    """Learned policies against the fixed yardstick opponents of ``selfplay.scripted`` in ONE ``evaluate_league`` pass over four segments of
    ``episodes`` slots each (``eval_env.num_envs == 4 * episodes``), in the order of ``BASELINE_SEGMENTS``: the learned cops against
    "evade" thieves and against "random" thieves, then "chase" cops and "random" cops against the learned thieves.  ``source``: a
    ``MAPPOTrainer`` (its current policies) or anything ``LeagueActor.load_set`` reads (a checkpoint file or its dict) holding every agent.
    ``actor``: a ``LeagueActor`` over ``eval_env`` with at least one set per agent to reuse (else one is built: ``fused`` as in
    ``LeagueActor.from_env``).  Returns {"segments": names, "episodes", "cop_wins", "thief_wins", "timeouts", "mean_length" (lists in
    segment order), "cop_win_rate", "ticks"}."""
    from .actor import LeagueActor
    agents = list(eval_env.possible_agents)
    if eval_env.num_envs != 4 * episodes or episodes < 1:
        raise ValueError(f"evaluate_against_scripts plays 4 segments of {episodes} episodes: the env must have {4 * episodes} slots, not {eval_env.num_envs}")
    if actor is None:
        actor = LeagueActor.from_env(eval_env, len(agents), fused=fused)
    if actor.sets < len(agents) or list(actor.agents) != agents:
        raise ValueError(f"the actor must cover {agents} with at least {len(agents)} sets")
    for g, a in enumerate(agents):
        actor.load_set(g, {a: source.agent_models(a)} if isinstance(source, MAPPOTrainer) else source, a)
    own = {a: g for g, a in enumerate(agents)}
    cop = lambda a: a.startswith("cop")
    who = [{a: own[a] if cop(a) else "evade" for a in agents}, {a: own[a] if cop(a) else "random" for a in agents},
           {a: "chase" if cop(a) else own[a] for a in agents}, {a: "random" if cop(a) else own[a] for a in agents}]
    actor.set_matchups([(s * episodes, (s + 1) * episodes, w) for s, w in enumerate(who)])
    res = evaluate_league(eval_env, actor, frame_skip=frame_skip, greedy=greedy)
    length = res["length"].float().view(4, episodes).mean(dim=1).tolist()
    return {"segments": list(BASELINE_SEGMENTS), "episodes": res["episodes"], "cop_wins": res["cop_wins"], "thief_wins": res["thief_wins"],
            "timeouts": res["timeouts"], "mean_length": length, "cop_win_rate": [c / episodes for c in res["cop_wins"]], "ticks": res["ticks"]}


NAVIGATOR_MATCHUPS = ("cops_vs_flee", "pursue_vs_thieves", "pursue_vs_flee", "pursue_vs_random", "random_vs_flee", "chase_vs_flee", "pursue_vs_evade")


@torch.no_grad()
def evaluate_against_navigators(eval_env, source, episodes: int, greedy: bool = False, frame_skip: int = 1, fused="kernel", actor=None,
                                cell: int = 16) -> Dict[str, object]:
    """The PRIVILEGED yardsticks of ``selfplay.navigators`` -- "pursue" cops and "flee" thieves, which read every agent's true position and
    the map -- against the learned policies, against each other, against "random" and against the scripted "chase" / "evade", in the order
    of ``NAVIGATOR_MATCHUPS``.  The match-ups are played one after another on ``eval_env`` (``num_envs == episodes``), the first episode of
    every slot each, by ``evaluate_league``'s rule.  ``source`` as in ``evaluate_against_scripts``; None skips the two learned rows.
    ``actor``: a ``LeagueActor`` over ``eval_env`` to reuse for the columns that are no navigator's (it needs a set per agent when
    ``source`` is given).  Returns {"segments": names, "episodes", "cop_wins", "thief_wins", "timeouts", "cop_win_rate", "mean_length",
    "mean_hops" (lists in match-up order), "ticks"}; ``mean_hops``: the mean of the navigators' ``nav_hops`` -- the hop count of the
    shortest path to the nearest opponent -- over their rows of the counted ticks that did not fall back (None without such a row)."""
    from .actor import LeagueActor
    from .navigators import NavigatorActor
    from ..navigation import NavField
    agents = list(eval_env.possible_agents)
    N = eval_env.num_envs
    if N != episodes or episodes < 1:
        raise ValueError(f"evaluate_against_navigators plays {episodes} episodes per match-up: the env must have {episodes} slots, not {N}")
    sets = len(agents) if source is not None else 1
    if actor is None:
        actor = LeagueActor.from_env(eval_env, sets, fused=fused)
    if actor.sets < sets or list(actor.agents) != agents:
        raise ValueError(f"the actor must cover {agents} with at least {sets} sets")
    own = {a: "random" for a in agents}
    if source is not None:
        for g, a in enumerate(agents):
            actor.load_set(g, {a: source.agent_models(a)} if isinstance(source, MAPPOTrainer) else source, a)
        own = {a: g for g, a in enumerate(agents)}
    cop = lambda a: a.startswith("cop")
    sides = {"cops": own, "thieves": own, "random": {a: "random" for a in agents}, "chase": {a: "chase" for a in agents},
             "evade": {a: "evade" for a in agents}}
    field = NavField.from_env(eval_env, cell)
    skip = _skip_kw(frame_skip)
    dev = actor.device
    out = {"segments": [], "episodes": [], "cop_wins": [], "thief_wins": [], "timeouts": [], "cop_win_rate": [], "mean_length": [], "mean_hops": [],
           "ticks": 0}
    for name in NAVIGATOR_MATCHUPS:
        cops, thieves = name.split("_vs_")
        if source is None and (cops == "cops" or thieves == "thieves"):       # the learned rows
            continue
        nav = {a: (cops if cop(a) else thieves) for a in agents}
        nav = {a: v for a, v in nav.items() if v in ("pursue", "flee")}
        # the league actor plays every column (a navigator's as "random"); the navigators then overwrite theirs
        actor.set_matchups([(0, N, {a: "random" if a in nav else sides[cops if cop(a) else thieves][a] for a in agents})])
        navigator = NavigatorActor(eval_env, nav, field=field)
        obs, _ = eval_env.reset()
        actor.reset()
        starts = torch.ones(N, dtype=torch.bool, device=dev)
        open_ = torch.ones(N, dtype=torch.bool, device=dev)
        winner = torch.full((N,), -1, dtype=torch.int8, device=dev)
        timeout = torch.zeros(N, dtype=torch.bool, device=dev)
        length = torch.zeros(N, dtype=torch.int32, device=dev)
        played = torch.zeros(N, dtype=torch.int32, device=dev)
        hop_sum = torch.zeros((), dtype=torch.int64, device=dev)
        hop_rows = torch.zeros((), dtype=torch.int64, device=dev)
        ticks = 0
        for _ in range(eval_env.max_step_count + 2):
            actions = actor.act(eval_env, starts, obs=obs, **({"greedy": True} if greedy else {}))
            navigator.act(eval_env, starts, actions=actions)
            counted = open_.view(1, N) & (navigator.nav_hops >= 0)
            hop_sum += torch.where(counted, navigator.nav_hops, torch.zeros_like(navigator.nav_hops)).sum()
            hop_rows += counted.sum()
            obs, _, terms, truncs, infos = eval_env.step(actions, **skip)
            ticks += 1
            done = terms[agents[0]]
            first = open_ & done
            winner = torch.where(first, infos["winner"].to(torch.int8), winner)
            timeout = torch.where(first, truncs[agents[0]], timeout)
            if skip:
                played = played + infos["ticks"]
            length = torch.where(first, played if skip else torch.full_like(length, ticks), length)
            open_ = open_ & ~done
            starts = done.clone()
            if not bool(open_.any()):                   # one host sync per tick, as evaluate_league
                break
        w, t = winner.cpu(), timeout.cpu()
        rows = int(hop_rows)
        out["segments"].append(name)
        out["episodes"].append(N)
        out["cop_wins"].append(int((w == 0).sum()))
        out["thief_wins"].append(int(((w == 1) & ~t).sum()))
        out["timeouts"].append(int(((w != 0) & t).sum()))
        out["cop_win_rate"].append(out["cop_wins"][-1] / N)
        out["mean_length"].append(float(length.float().mean()))
        out["mean_hops"].append(int(hop_sum) / rows if rows else None)
        out["ticks"] += ticks
    return out


def evaluate_agent_league(eval_env, actor, learned: MAPPOTrainer, archives: Dict[str, Path], tc: TrainingConfig, rng: random.Random, log=print,
                          learned_roles: Optional[Tuple[str, ...]] = None, frame_skip: int = 1) -> Dict[str, Dict[str, bool]]:
    """``evaluate_agent`` for the roles in ``learned_roles`` (default: cops, then thieves) in ONE pass of ``evaluate_league``: every newly
    trained role against its up to ``tc.num_opponents_to_evaluate`` distinct archived opponents, each match-up on its own segment of
    ``tc.n_trial_episodes`` slots of ``eval_env``.  ``actor``: a ``LeagueActor`` over ``eval_env`` with at least
    ``len(agents) * (1 + tc.num_opponents_to_evaluate)`` sets; ``eval_env`` has ``len(learned_roles) * num_opponents_to_evaluate *
    n_trial_episodes`` slots (segments that no opponent fills play at random and count nothing).  ``archives``: role -> its archive.
    The opponents are drawn by ``evaluate_agent``'s own sampling loop -- the same strategy, the same ``rng`` consumption per draw -- and one
    outcome per opponent is booked with ``archive.update_policy_win_rate`` in draw order.  Returns {learned role: {opponent file: opponent won}}.

    The ONE protocol difference to the sequential form: here all opponents of a role are drawn from the win rates as they stood BEFORE this
    evaluation; ``evaluate_agent`` draws opponent i + 1 after it has booked opponent i, so with PFSP its later draws see the earlier outcomes."""
    cop, thief = tc.cop_role_prefix, tc.thief_role_prefix
    learned_roles = (cop, thief) if learned_roles is None else tuple(learned_roles)
    K, E, agents = tc.num_opponents_to_evaluate, tc.n_trial_episodes, list(actor.agents)
    assert eval_env.num_envs == actor.N == len(learned_roles) * K * E, (eval_env.num_envs, actor.N, len(learned_roles), K, E)
    assert actor.sets >= len(agents) * (1 + K), (actor.sets, len(agents), K)
    role_of = {a: a.split("_")[0] for a in agents}
    own = {a: g for g, a in enumerate(agents)}                            # sets 0 .. G - 1: the newly trained policies
    drawn = {}
    for learned_role in learned_roles:
        opponent_role = thief if learned_role == cop else cop
        seen, paths = set(), []
        for i in range(K):
            path = _draw_new_opponent(archives[opponent_role], opponent_role, tc, rng, seen)
            if path is None:
                log(f"[self-play] no new distinct {opponent_role} opponent for evaluation round {i + 1}/{K}")
                break
            seen.add(Path(path).name)
            paths.append(path)
        drawn[learned_role] = (opponent_role, paths)
    results: Dict[str, Dict[str, bool]] = {r: {} for r in learned_roles}
    if not any(paths for _, paths in drawn.values()):
        return results
    for a in agents:
        actor.load_set(own[a], {a: learned.agent_models(a)}, a)
    segments, quota, cells, nxt = [], [], [], len(agents)
    for r, learned_role in enumerate(learned_roles):
        opponent_role, paths = drawn[learned_role]
        for i, path in enumerate(paths):
            sd = torch.load(path, map_location="cpu", weights_only=True)
            who = {}
            for a in agents:
                if role_of[a] == opponent_role:
                    actor.load_set(nxt, sd, a)
                    who[a], nxt = nxt, nxt + 1
                else:
                    who[a] = own[a]
            lo = (r * K + i) * E
            segments.append((lo, lo + E, who))
            quota.append(E)
            cells.append((learned_role, Path(path).name))
        lo, hi = (r * K + len(paths)) * E, (r + 1) * K * E
        if lo < hi:                                                       # fewer opponents than segments: these slots fill the env
            segments.append((lo, hi, {a: "random" for a in agents}))
            quota.append(0)
            cells.append(None)
    actor.set_matchups(segments)
    res = evaluate_league(eval_env, actor, quota, frame_skip=frame_skip)
    w = res["winner"].cpu()
    for (lo, hi, _), cell in zip(segments, cells):
        if cell is None:
            continue
        learned_role, name = cell
        cop_rate, thief_rate = float((w[lo:hi] == 0).sum()) / E, float((w[lo:hi] == 1).sum()) / E
        opponent_won = (thief_rate > cop_rate) if learned_role == cop else (cop_rate > thief_rate)
        archive.update_policy_win_rate(archives[drawn[learned_role][0]], name, opponent_won, tc.win_rate_buffer_size)
        results[learned_role][name] = opponent_won
        log(f"[self-play]   {learned_role} vs {name}: cop {cop_rate:.2f} thief {thief_rate:.2f} -> opponent {'won' if opponent_won else 'lost'}")
    return results


def even_segments(n: int, parts: int):
    """[(start, stop)] of ``parts`` contiguous segments of ``n`` rows whose sizes differ by at most one (the longer ones first)."""
    assert 1 <= parts <= n, (n, parts)
    base, extra = divmod(n, parts)
    bounds = [0]
    for i in range(parts):
        bounds.append(bounds[-1] + base + (i < extra))
    return list(zip(bounds[:-1], bounds[1:]))


def _training_opponents(tc: TrainingConfig) -> int:
    """``tc.num_training_opponents``, checked where role training reads it (the simultaneous loop never does)."""
    k = tc.num_training_opponents
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 32:
        raise ValueError(f"TrainingConfig.num_training_opponents must be an integer in 1..32, got {k!r}")
    return k


def _role_actor(env, trainer: MAPPOTrainer, sets: int, agents=None, seed: int = 0):
    """A ``LeagueActor`` over ``env`` in the trainer's number formats; the one-launch kernel where it applies, the per-layer chain elsewhere."""
    from .actor import LeagueActor
    tcfg = trainer.tcfg
    return LeagueActor.from_env(env, sets, fused="kernel", compute_bf16=tcfg.compute_bf16, normalize_inputs=tcfg.normalize_inputs,
                                recurrent=tcfg.recurrent, seed=seed, device=trainer.device, agents=agents)


def train_role_league(trainer: MAPPOTrainer, env, eval_env, learned_role: str, opponent_role: str, archives: Dict[str, Path], tc: TrainingConfig,
                      rng: random.Random, log=print, iteration: int = 0, out_dir: Optional[Path] = None, total_iterations: Optional[int] = None,
                      timesteps: Optional[int] = None, train_actor=None, eval_actor=None) -> Dict[str, object]:
    """One role-training phase -- the reference's ``train_role`` / ``_orchestrate_training_phase`` (``agent_learning_utils.py:22-169``,
    ``orchestration.py:31-97``: fictitious play against a frozen opponent drawn from the opponent archive) -- against up to
    ``tc.num_training_opponents`` archived opponents AT ONCE, each on its own contiguous segment of the training env's slots:

    1. ``learned_role`` continues from the latest entry of its archive (weights only; its Adam state starts fresh);
    2. up to ``num_training_opponents`` DISTINCT ``opponent_role`` policies are drawn by ``tc.policy_sample_strategy`` (``_draw_new_opponent``);
       fewer archived entries give fewer segments, an empty archive one segment of ``"random"``;
    3. the env's slots are cut into that many segments (``even_segments``), the opponents go into the bank of ``train_actor`` (a ``LeagueActor`` over
       the opponent role's agents of ``env``; built here when None) and the trainer hands the role to it (``MAPPOTrainer.set_opponent``);
    4. ``trainer.train(timesteps)``: the learner alone is updated;
    5. booking as the reference does after a phase (``agent_learning_utils.py:135-151``), for all opponents in ONE ``evaluate_league`` pass on
       ``opponents x tc.n_trial_episodes`` slots of ``eval_env`` through ``eval_actor`` (a ``LeagueActor`` over all agents of ``eval_env`` with at least
       ``learned agents + opponents x opponent agents`` sets; built here when None): per opponent ONE outcome -- the archived opponent won more
       episodes than the learner -- into its entry of the opponent archive's ``win_rates.json``; nothing for ``"random"``;
    6. ``trainer.state_dict()`` -- the learned role's agents: the opponent role is the actor's -- is saved as ``{role}_iter_{i}_full_agent.pt`` under
       ``out_dir`` (default: the parent of the role's archive) and added to THAT role's archive only (``orchestration.py:83-93``); the role goes
       back to the trainer.

    The trainer must hold one learner per role (``MAPPOTrainer(..., split_roles=True)`` or unlike role configurations).  Differences to the
    reference: many opponents per phase; all of them drawn before the phase (from the win rates as they stood then); ``"random"`` against an
    empty archive, where the reference leaves the opponent role's freshly initialised networks in play.
    Returns ``{"role", "opponents" (file names or ["random"]), "segments", "outcomes" {file: opponent won}, "stats", "checkpoint"}``."""
    if learned_role not in trainer.roles or opponent_role not in trainer.roles:
        raise ValueError(f"role training needs one learner per role (MAPPOTrainer(..., split_roles=True)); this trainer's learners are {sorted(trainer.roles)}")
    K, E, N = _training_opponents(tc), tc.n_trial_episodes, trainer.N
    learner, opp_agents = trainer.roles[learned_role], list(trainer.roles[opponent_role].agents)
    # ---- 1. the learner's latest archived weights, a fresh Adam
    ck = archive.sample_policy_from_archive(archives[learned_role], learned_role, "latest")
    if ck:
        trainer.load_state_dict(torch.load(ck, map_location=trainer.device, weights_only=True), roles=[learned_role], optimizer=False)
    learner.m.zero_(); learner.v.zero_(); learner.steps.zero_()
    # ---- 2. the opponents, all drawn from the win rates as they stand now
    seen, paths = set(), []
    for i in range(min(K, N)):
        path = _draw_new_opponent(archives[opponent_role], opponent_role, tc, rng, seen)
        if path is None:
            break
        seen.add(Path(path).name)
        paths.append(path)
    names = [Path(p).name for p in paths]
    # ---- 3. segments, bank, hand-over
    G = len(opp_agents)
    if train_actor is None:
        train_actor = _role_actor(env, trainer, K * G, agents=opp_agents)
    if train_actor.sets < max(1, len(paths)) * G:
        raise ValueError(f"the training actor's bank of {train_actor.sets} sets cannot hold {len(paths)} opponents x {G} agents")
    bounds = even_segments(N, max(1, len(paths)))
    loaded = [torch.load(p, map_location="cpu", weights_only=True) for p in paths]
    matchups = []
    for i, (lo, hi) in enumerate(bounds):
        who = {}
        for g, a in enumerate(opp_agents):
            if paths:
                train_actor.load_set(i * G + g, loaded[i], a)
                who[a] = i * G + g
            else:
                who[a] = "random"
        matchups.append((lo, hi, who))
    train_actor.set_matchups(matchups)
    trainer.set_opponent(opponent_role, train_actor)
    result: Dict[str, object] = {"role": learned_role, "opponents": names or ["random"], "segments": bounds, "outcomes": {}}
    try:
        trainer.reset_episodes()
        log(f"[self-play] iteration {iteration}: training {learned_role}s against {', '.join(names) if names else 'random ' + opponent_role + 's'}")
        # ---- 4. the phase
        result["stats"] = trainer.train(trainer.tcfg.timesteps if timesteps is None else timesteps)
        # ---- 5. one outcome per archived opponent
        if paths:
            agents = list(eval_env.possible_agents)
            own = [a for a in agents if a in learner.agents]
            if eval_actor is None:
                eval_actor = _role_actor(eval_env, trainer, len(own) + K * G, seed=1)
            if eval_env.num_envs < len(paths) * E or eval_actor.sets < len(own) + len(paths) * G:
                raise ValueError(f"booking {len(paths)} opponents x {E} episodes needs {len(paths) * E} evaluation slots and {len(own) + len(paths) * G} sets: "
                                 f"the evaluation env has {eval_env.num_envs}, the actor's bank {eval_actor.sets}")
            for k, a in enumerate(own):
                eval_actor.load_set(k, {a: trainer.agent_models(a)}, a)
            segs, quota = [], []
            for i, sd in enumerate(loaded):
                who = {a: k for k, a in enumerate(own)}
                for g, a in enumerate(opp_agents):
                    eval_actor.load_set(len(own) + i * G + g, sd, a)
                    who[a] = len(own) + i * G + g
                segs.append((i * E, (i + 1) * E, who))
                quota.append(E)
            if len(paths) * E < eval_env.num_envs:                         # slots no opponent fills: they play at random and count nothing
                segs.append((len(paths) * E, eval_env.num_envs, {a: "random" for a in agents}))
                quota.append(0)
            eval_actor.set_matchups(segs)
            w = evaluate_league(eval_env, eval_actor, quota, frame_skip=trainer.tcfg.frame_skip)["winner"].cpu()
            for i, name in enumerate(names):
                cop_rate, thief_rate = float((w[i * E:(i + 1) * E] == 0).sum()) / E, float((w[i * E:(i + 1) * E] == 1).sum()) / E
                opponent_won = (thief_rate > cop_rate) if learned_role == tc.cop_role_prefix else (cop_rate > thief_rate)
                archive.update_policy_win_rate(archives[opponent_role], name, opponent_won, tc.win_rate_buffer_size)
                result["outcomes"][name] = opponent_won
                log(f"[self-play]   {learned_role} vs {name}: cop {cop_rate:.2f} thief {thief_rate:.2f} -> opponent {'won' if opponent_won else 'lost'}")
        # ---- 6. the learned role's checkpoint, into its own archive only
        out_dir = Path(archives[learned_role]).parent if out_dir is None else Path(out_dir)
        ck = out_dir / f"{learned_role}_iter_{iteration}_full_agent.pt"
        torch.save(trainer.state_dict(), ck)
        if iteration % tc.archive_save_interval == 0 or (total_iterations is not None and iteration == total_iterations - 1):
            archive.add_policy_to_archive(str(ck), archives[learned_role], iteration, learned_role)
        result["checkpoint"] = str(ck)
    finally:
        trainer.set_opponent(opponent_role, None)
    return result


def _role_training_iterations(its, trainer, env, eval_env, arch, tc, rng, log, out_dir, train_actors, eval_actor, episode_stats: bool,
                              skip_archived: bool = False):
    """``run_self_play(role_training=True)``'s loop: per iteration the cop phase, then the thief phase (``orchestration.py``'s order).
    ``skip_archived`` (a resumed run): a phase whose role's archive already holds this iteration is not played again."""
    cop, thief = tc.cop_role_prefix, tc.thief_role_prefix
    phase_file = out_dir / "role_training.json"
    phase_log = json.loads(phase_file.read_text()) if episode_stats and its and its[0] > 0 and phase_file.exists() else []
    history = []
    for it in its:
        phases = []
        for learned_role, opponent_role in ((cop, thief), (thief, cop)):
            if skip_archived and (Path(arch[learned_role]) / f"{learned_role}_iter_{it}.pt").exists():
                log(f"[self-play] iteration {it}: the {learned_role}s' phase is in the archive already")
                continue
            ph = train_role_league(trainer, env, eval_env, learned_role, opponent_role, arch, tc, rng, log, iteration=it, out_dir=out_dir,
                                   total_iterations=its[-1] + 1, timesteps=trainer.tcfg.timesteps, train_actor=train_actors[opponent_role],
                                   eval_actor=eval_actor)
            phases.append(ph)
            log(f"[self-play] iteration {it}: saved {Path(ph['checkpoint']).name}; booked {len(ph['outcomes'])} {opponent_role} opponent(s)")
            if episode_stats:
                keys = ("episodes", "cop_wins", "thief_wins", "timeouts", "mean_length")
                phase_log.append({"iteration": it, "role": learned_role, "opponents": ph["opponents"], "slots": [list(b) for b in ph["segments"]],
                                  "segments": [{k: seg[k] for k in keys} for seg in ph["stats"].get("segments", [])]})
                phase_file.write_text(json.dumps(phase_log, indent=1))
        history.append({"iteration": it, "phases": phases, "evaluations": {ph["role"]: ph["outcomes"] for ph in phases},
                        "stats": {ph["role"]: ph["stats"] for ph in phases}})
    return history


def run_self_play(map_name: str, num_envs: int, out_dir: Path, iterations: Optional[int] = None,
                  training: Optional[TrainingConfig] = None, trainer_cfg: Optional[TrainerConfig] = None,
                  role_cfg: Optional[Dict[str, RoleConfig]] = None, num_rays: int = 64, n_cops: Optional[int] = None,
                  n_thieves: Optional[int] = None, max_step_count: int = 2000, eval_envs: Optional[int] = None,
                  seed: int = 0, device=None, resume: bool = True, log=print, env_factory=None,
                  query_order: str = "index", tracked_eval: bool = False, episode_stats: bool = False,
                  fused_eval: bool = False, league_eval: bool = False, role_training: bool = False,
                  fused_collect: bool = False, value_norm: bool = False, position_stats: Optional[int] = None,
                  lr_schedule: str = "constant", lr_final: Optional[float] = None, lr_kl_target: Optional[float] = None,
                  entropy_final: Optional[float] = None, ratio_clip_final: Optional[float] = None,
                  baseline_eval: bool = False, baseline_episodes: int = 64, navigator_eval: bool = False,
                  navigator_episodes: int = 64, geodesic_shaping: float = 0.0, shaping_scale_thief: Optional[float] = None,
                  shaping_cap: Optional[int] = None, spawn_curriculum: Optional[Tuple[int, int]] = None, curriculum_fraction: float = 1.0,
                  curriculum_adapt: Optional[Tuple[float, float]] = None, curriculum_step: int = 1, curriculum_max: int = 64,
                  separation_eval: Optional[List[Tuple[int, int]]] = None, separation_episodes: int = 64) -> Dict[str, object]:
    """The self-play loop.  ``resume``: continue after the highest iteration found in the archives ("latest").
    ``query_order``: the visiting order of the walls in the envs' segment queries (``VecCopsEnv``: "index" or "chipmunk").
    ``max_step_count``: 2000, what the reference's driver passes (``self_play_driver.py:34``).
    ``env_factory(num_envs, seed[, env_id_offset])``: build the envs some other way (the CPU tests pass a stand-in env with the
    same surface).
    ``fused_eval``: the evaluator is a ``PolicyActor`` instead of a second ``MAPPOTrainer``: policy blocks and recurrent state only, and on a
    GPU the act tick of all policies is one launch (``include/cat_act.h``).
    ``league_eval``: both roles' evaluations of an iteration share ONE pass (``evaluate_agent_league``) through a ``LeagueActor`` on an
    evaluation env of ``2 x num_opponents_to_evaluate x n_trial_episodes`` slots (``eval_envs``, if given, must be that number); the log
    lines and ``win_rates.json`` keep their form.  Not with ``tracked_eval``.
    ``tracked_eval``: the evaluation env is built with ``track_episodes=True`` and evaluation goes through
    ``evaluate_agents_tracked``.  ``episode_stats``: the training env is built with ``track_episodes=True``, the trainer reports the
    training episodes (``TrainerConfig.episode_stats``), every iteration's log line carries their win rate and mean length, and rank
    0 writes ``episode_stats.json``, one entry per iteration (in a data-parallel run: the episodes of rank 0's shard of the envs).  Envs of an ``env_factory`` must bring their own ``episode_tracker``.

    ``role_training``: the reference's OTHER training mode (``train_role``: fictitious play) instead of the simultaneous one -- per iteration a cop
    phase, then a thief phase (``train_role_league``): the role continues from its archive, trains against up to
    ``training.num_training_opponents`` archived opponents at once (drawn by the configured strategy; "random" against an empty archive),
    one outcome per opponent is booked, and ``{role}_iter_{i}_full_agent.pt`` goes into that role's archive only.  The trainer then holds
    one learner per role and the evaluation env has ``num_training_opponents x n_trial_episodes`` slots (``eval_envs``, if given, must be
    that number); ``fused_eval`` / ``league_eval`` have nothing to choose (the booking is one ``evaluate_league`` pass).  With
    ``episode_stats`` every phase's per-opponent training figures go into ``role_training.json``.  Not with ``tracked_eval``, and not in a
    data-parallel job (ValueError on every rank before any collective).  ``resume`` continues after the lowest iteration that BOTH roles'
    archives hold and skips a phase whose role has that iteration archived, so a run stopped between the cop and the thief phase of an
    iteration plays the missing thief phase first.

    ``fused_collect``: the training rollouts go through the one-launch collect tick (``TrainerConfig.fused_collect``; ValueError from the
    trainer where it cannot apply).  The evaluator is not affected.

    ``value_norm``: the critics train on returns normalised by running per-agent moments (``TrainerConfig.value_norm``); the joint
    checkpoints then carry each agent's moments (``vn_state``) beside its value network.

    ``geodesic_shaping=W`` (with ``shaping_scale_thief``, ``shaping_cap``): the learners' rewards take the geodesic potential-based shaping
    term of ``TrainerConfig.geodesic_shaping``; the training env is then built with ``final_positions=True`` (an ``env_factory``'s env must
    bring it along: ValueError from the trainer otherwise).  Evaluation, the archives and the booked outcomes see the env's own rewards only.

    ``spawn_curriculum=(lo, hi)`` (with ``curriculum_fraction``, ``curriculum_adapt``, ``curriculum_step``, ``curriculum_max``): the geodesic
    start-state curriculum of ``TrainerConfig.spawn_curriculum``.  ONLY the training env gets the spawner: the evaluation envs keep the map's
    own spawn, so ``win_rates.json`` stays comparable.  Single process only (ValueError in a data-parallel job, on every rank before any
    collective).  The joint checkpoints carry the band; a resumed run starts it from the configuration.
    ``separation_eval=[(lo, hi), ...]``: after every iteration rank 0 runs ``evaluate_by_separation`` -- the cops' win rate as a function of
    the initial geodesic separation -- on an env of its own with ``len(bands) * separation_episodes`` slots and appends the result to
    ``separation.json``.  The simultaneous mode only.  Off, nothing of it is built and no random number is drawn for it.

    ``lr_schedule`` ("constant", "linear" with ``lr_final``, "kl_adaptive" with ``lr_kl_target``), ``entropy_final``, ``ratio_clip_final``: the
    schedules of ``RoleConfig``, put into both roles' configurations.  A role configuration that leaves ``schedule_updates`` at 0 gets the
    number of updates this call will make for it (``planned_updates``), so that a linear anneal ends with the run.  The schedule runs on
    through the iterations (``reset_optimizers`` renews Adam, not the schedule); the log line of an iteration shows the learning rates.

    ``position_stats=CELL``: the evaluation env is built with ``track_positions=CELL`` and after every iteration's evaluation rank 0 writes
    the heatmaps of that evaluation's rows (``render.write_heatmaps``) into ``positions_iter_{i}/`` of the run directory, then clears the
    maps.  The simultaneous mode only (ValueError with ``role_training``); envs of an ``env_factory`` must bring their own ``position_tracker``.
    ``baseline_eval``: after every iteration's evaluation rank 0 plays the trained policies against the fixed yardsticks -- the scripted
    "chase" / "evade" opponents of ``scripted.py`` and "random" -- in one ``evaluate_against_scripts`` pass on an env of its own with
    ``4 * baseline_episodes`` slots, and appends the result to ``baselines.json`` of the run directory.  The simultaneous mode only.  Off,
    nothing of it is built and no random number is drawn for it.
    ``navigator_eval``: the same for the PRIVILEGED navigator yardsticks (``navigators.py``: "pursue" / "flee" read true positions and the
    map): after every iteration rank 0 runs ``evaluate_against_navigators`` on an env of its own with ``navigator_episodes`` slots and appends
    the result to ``navigators.json``.  The simultaneous mode only.  Off, nothing of it is built and no random number is drawn for it.

    With an initialised ``torch.distributed`` group of W > 1 ranks this is ONE data-parallel job: ``num_envs`` is the TOTAL,
    rank r simulates ``shard_envs(num_envs, r, W)``; the trainer all-reduces its gradient | KL buffer every optimiser step (all
    ranks hold identical parameters at all times); rank 0 alone evaluates and writes files, the others wait and read them."""
    import torch.distributed as dist
    from ..sharding import shard_envs
    if league_eval and tracked_eval:
        raise ValueError("league_eval plays through evaluate_league (one poll per tick): it cannot be combined with tracked_eval")
    if baseline_eval and (role_training or baseline_episodes < 1):
        raise ValueError("baseline_eval belongs to the simultaneous loop (not role_training) and needs baseline_episodes >= 1")
    if navigator_eval and (role_training or navigator_episodes < 1):
        raise ValueError("navigator_eval belongs to the simultaneous loop (not role_training) and needs navigator_episodes >= 1")
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    chief = rank == 0
    if role_training and multi:                  # every rank sees the same two facts: all refuse, none is left in a collective
        raise ValueError("role_training is a single-process mode: multi-rank role training is not supported")
    if role_training and position_stats is not None:
        raise ValueError("position_stats writes the heatmaps of the simultaneous mode's evaluations: it cannot be combined with role_training")
    if (spawn_curriculum is not None or separation_eval) and multi:
        raise ValueError("spawn_curriculum / separation_eval are single-process options: a data-parallel job cannot take them")
    if separation_eval and (role_training or separation_episodes < 1):
        raise ValueError("separation_eval belongs to the simultaneous loop (not role_training) and needs separation_episodes >= 1")
    if role_training and tracked_eval:
        raise ValueError("role_training books its outcomes through evaluate_league (one poll per tick): it cannot be combined with tracked_eval")

    def sync(ok: bool = True, what: str = ""):
        """File hand-over between rank 0 and the others: a MIN all-reduce of an ok flag instead of a bare barrier, so that a failure
        of rank 0 while it evaluates or writes reaches every rank at once (they raise too) instead of leaving them in a collective
        until the backend's watchdog fires.  The group is opened with a generous timeout (``init_ranks``): rank 0's evaluation
        (2000-tick episodes against several archived opponents) runs while the others wait here."""
        if multi:
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0 and ok:
                raise RuntimeError(f"self-play: rank 0 failed {what or 'in its rank-0-only section'}; this rank ({rank}) stops with it")
    tc = training or TrainingConfig()
    iterations = tc.num_self_play_iterations if iterations is None else iterations
    # TrainerConfig's 128-tick rollouts: with 16-tick rollouts the cops' win rate against random thieves stays at its untrained
    # 10 % for 262 M env-steps, with 128 it rises (profiles/r02_learning_curves.txt); the reference collects 4096 ticks per update
    trainer_cfg = trainer_cfg or TrainerConfig(timesteps=tc.training_timesteps_per_role_training)
    if episode_stats:
        trainer_cfg = dataclasses.replace(trainer_cfg, episode_stats=True)
    if fused_collect:
        trainer_cfg = dataclasses.replace(trainer_cfg, fused_collect=True)
    if value_norm:
        trainer_cfg = dataclasses.replace(trainer_cfg, value_norm=True)
    if geodesic_shaping or shaping_scale_thief:
        trainer_cfg = dataclasses.replace(trainer_cfg, geodesic_shaping=geodesic_shaping, shaping_scale_thief=shaping_scale_thief,
                                          **({} if shaping_cap is None else {"shaping_cap": shaping_cap}))
    if spawn_curriculum is not None:
        trainer_cfg = dataclasses.replace(trainer_cfg, spawn_curriculum=tuple(spawn_curriculum), curriculum_fraction=curriculum_fraction,
                                          curriculum_adapt=None if curriculum_adapt is None else tuple(curriculum_adapt),
                                          curriculum_step=curriculum_step, curriculum_max=curriculum_max)
    shaped = any(trainer_cfg.shaping_scales)
    out_dir = Path(out_dir)
    arch = {tc.cop_role_prefix: out_dir / "cops", tc.thief_role_prefix: out_dir / "thieves"}
    if chief:
        for p in arch.values():
            p.mkdir(parents=True, exist_ok=True)
    sync()
    n_eval = eval_envs or tc.n_trial_episodes
    if league_eval:
        n_eval = 2 * tc.num_opponents_to_evaluate * tc.n_trial_episodes
        if eval_envs not in (None, n_eval):
            raise ValueError(f"league_eval plays on 2 x {tc.num_opponents_to_evaluate} opponents x {tc.n_trial_episodes} episodes = {n_eval} slots, not eval_envs={eval_envs}")
    if role_training:
        n_eval = _training_opponents(tc) * tc.n_trial_episodes
        if eval_envs not in (None, n_eval):
            raise ValueError(f"role_training books on {tc.num_training_opponents} opponents x {tc.n_trial_episodes} episodes = {n_eval} slots, not eval_envs={eval_envs}")
    train_factory = eval_factory = env_factory
    if env_factory is None:
        preset = load_preset(map_name, n_cops, n_thieves)
        make = lambda track, **more: (lambda n, s, off=0: VecCopsEnv(preset, n, num_rays=num_rays, max_step_count=max_step_count, seed=s, device=device,
                                                                     env_id_offset=off, query_order=query_order, track_episodes=track, **more))
        env_factory = train_factory = make(episode_stats, **({"final_positions": True} if shaped else {}))    # the shaper reads where episodes ended
        eval_factory = make(tracked_eval)
        if position_stats is not None:
            eval_factory = lambda n, s, off=0: VecCopsEnv(preset, n, num_rays=num_rays, max_step_count=max_step_count, seed=s, device=device,
                                                          env_id_offset=off, query_order=query_order, track_episodes=tracked_eval,
                                                          track_positions=position_stats, final_positions=True)
    n_local, offset = shard_envs(num_envs, rank, world)
    if multi:
        # checked on EVERY rank from the same numbers, so that all of them refuse together (a rank that raised alone would leave the others in the
        # trainer's first all-reduce): the smallest shard must still fill every role's minibatches
        smallest = min(shard_envs(num_envs, r, world)[0] for r in range(world))
        windows = max(1, trainer_cfg.horizon // min(trainer_cfg.bptt, trainer_cfg.horizon))
        need = max(c.mini_batches for c in (role_cfg or {"cop": CFG_AGENT, "thief": CFG_AGENT}).values())
        if smallest * windows < need:
            raise ValueError(f"{num_envs} envs over {world} ranks leave a rank {smallest} env(s) = {smallest * windows} training sequences per update, "
                             f"fewer than the {need} minibatches of the role configuration")
    takes_offset = len(inspect.signature(env_factory).parameters) >= 3
    if multi and not takes_offset:
        raise TypeError("a data-parallel run needs env_factory(num_envs, seed, env_id_offset): the ranks must simulate different envs")
    env = train_factory(n_local, seed, offset) if takes_offset else train_factory(n_local, seed)
    eval_env = eval_factory(n_eval, seed + 7919)         # every rank builds one (the evaluator's shapes); only rank 0 plays on it
    for what, e, attr in (("tracked_eval", eval_env, "episode_tracker"), ("episode_stats", env, "episode_stats")):
        if {"tracked_eval": tracked_eval, "episode_stats": episode_stats}[what] and not hasattr(e, attr):
            raise TypeError(f"{what}=True needs envs with an {attr!r} (VecCopsEnv(track_episodes=True)); the env_factory's have none")
    if position_stats is not None and not hasattr(eval_env, "position_tracker"):
        raise TypeError("position_stats needs an evaluation env with a 'position_tracker' (VecCopsEnv(track_positions=CELL)); the env_factory's has none")
    if position_stats is not None:
        eval_env.position_tracker.clear()
    role_cfg = role_cfg or {"cop": CFG_AGENT, "thief": CFG_AGENT}        # self_play_driver.py passes CFG_AGENT
    asked = {k: v for k, v in (("lr_schedule", lr_schedule), ("lr_final", lr_final), ("lr_kl_target", lr_kl_target),
                               ("entropy_final", entropy_final), ("ratio_clip_final", ratio_clip_final)) if v not in (None, "constant")}
    if asked:
        role_cfg = {r: dataclasses.replace(c, **asked) for r, c in role_cfg.items()}
        role_cfg = {r: c if c.schedule_updates else dataclasses.replace(c, schedule_updates=planned_updates(iterations, trainer_cfg, c))
                    for r, c in role_cfg.items()}
    trainer = MAPPOTrainer(env, role_cfg, trainer_cfg, seed=seed, **({"split_roles": True} if role_training else {}))
    if role_training:  # per role a bank of archived opponents over the training env; one bank over the evaluation env for the booking
        evaluator = None
        by_role = {r: [a for a in trainer.agents if a.split("_")[0] == r] for r in arch}
        train_actors = {r: _role_actor(env, trainer, tc.num_training_opponents * len(by_role[r]), agents=by_role[r], seed=seed + 2) for r in arch}
        eval_actor = _role_actor(eval_env, trainer, len(trainer.agents) * (1 + tc.num_training_opponents), seed=seed + 1)
    elif league_eval:  # a bank of policy blocks: the trained agents' and every drawn opponent's (include/cat_act.h, cat_act_league_step)
        from .actor import LeagueActor
        evaluator = LeagueActor.from_env(eval_env, len(eval_env.possible_agents) * (1 + tc.num_opponents_to_evaluate), fused="kernel",
                                         compute_bf16=trainer_cfg.compute_bf16, normalize_inputs=trainer_cfg.normalize_inputs,
                                         recurrent=trainer_cfg.recurrent, seed=seed + 1, device=trainer.device)
    elif fused_eval:   # policy blocks and recurrent state only; on a GPU the act tick is one launch (include/cat_act.h)
        from .actor import PolicyActor
        evaluator = PolicyActor.from_checkpoint(None, eval_env, fused="kernel", compute_bf16=trainer_cfg.compute_bf16, normalize_inputs=trainer_cfg.normalize_inputs,
                                                recurrent=trainer_cfg.recurrent, seed=seed + 1, device=trainer.device)
    else:
        evaluator = MAPPOTrainer(eval_env, role_cfg, dataclasses.replace(trainer_cfg, graph_rollout=False, graph_update=False, fused_collect=False,
                                                                         geodesic_shaping=0.0, shaping_scale_thief=None,
                                                                         curriculum_adapt=None, spawn_curriculum=None),
                                 seed=seed + 1)
    baseline_env = baseline_actor = None
    baseline_log = []
    if baseline_eval and chief:    # the fixed yardsticks (scripted.py): four segments of baseline_episodes slots, one pass per iteration
        from .actor import LeagueActor
        baseline_env = eval_factory(4 * baseline_episodes, seed + 7927)
        baseline_actor = LeagueActor.from_env(baseline_env, len(baseline_env.possible_agents), fused="kernel", compute_bf16=trainer_cfg.compute_bf16,
                                              normalize_inputs=trainer_cfg.normalize_inputs, recurrent=trainer_cfg.recurrent, seed=seed + 3,
                                              device=trainer.device)
    navigator_env = navigator_actor = None
    navigator_log = []
    if navigator_eval and chief:   # the privileged yardsticks (navigators.py): the match-ups one after another on navigator_episodes slots
        from .actor import LeagueActor
        navigator_env = eval_factory(navigator_episodes, seed + 7933)
        navigator_actor = LeagueActor.from_env(navigator_env, len(navigator_env.possible_agents), fused="kernel", compute_bf16=trainer_cfg.compute_bf16,
                                               normalize_inputs=trainer_cfg.normalize_inputs, recurrent=trainer_cfg.recurrent, seed=seed + 5,
                                               device=trainer.device)
    separation_env = separation_actor = None
    separation_log = []
    if separation_eval and chief:  # the cops' win rate by initial geodesic separation: one segment of separation_episodes slots per band
        from .actor import LeagueActor
        separation_env = eval_factory(len(separation_eval) * separation_episodes, seed + 7937)
        separation_actor = LeagueActor.from_env(separation_env, len(separation_env.possible_agents), fused="kernel", compute_bf16=trainer_cfg.compute_bf16,
                                                normalize_inputs=trainer_cfg.normalize_inputs, recurrent=trainer_cfg.recurrent, seed=seed + 9,
                                                device=trainer.device)
    rng = random.Random(seed)
    start = 0
    if resume:
        latest = [archive.get_latest_policy_from_archive(arch[r], r) for r in arch]
        its = [int(Path(p).stem.split("_")[-1]) for p in latest if p]
        start = max(its) + 1 if its else 0
        if role_training:        # the phases archive one role each: a run that was stopped between the two of an iteration has them one
            # apart, and goes on AT that iteration, where the loop skips the phase the archive already holds
            start = min(int(Path(p).stem.split("_")[-1]) if p else -1 for p in latest) + 1
    history, episode_log = [], []
    stats_file = out_dir / "episode_stats.json"
    if episode_stats and chief and start > 0 and stats_file.exists():
        episode_log = json.loads(stats_file.read_text())
    baselines_file = out_dir / "baselines.json"
    if baseline_env is not None and start > 0 and baselines_file.exists():
        baseline_log = json.loads(baselines_file.read_text())
    navigators_file = out_dir / "navigators.json"
    if navigator_env is not None and start > 0 and navigators_file.exists():
        navigator_log = json.loads(navigators_file.read_text())

    separation_file = out_dir / "separation.json"
    if separation_env is not None and start > 0 and separation_file.exists():
        separation_log = json.loads(separation_file.read_text())

    def finish():
        digest = trainer.param_digest()
        if separation_env is not None:
            separation_env.close()
        env.close()
        eval_env.close()
        if baseline_env is not None:
            baseline_env.close()
        if navigator_env is not None:
            navigator_env.close()
        return {"iterations": history, "param_digest": digest, "archives": {r: str(p) for r, p in arch.items()}, "rank": rank, "world": world,
                "envs_local": n_local, "env_id_offset": offset}

    if role_training:
        history = _role_training_iterations(range(start, start + iterations), trainer, env, eval_env, arch, tc, rng, log, out_dir, train_actors,
                                            eval_actor, episode_stats, skip_archived=resume)
        return finish()
    for it in range(start, start + iterations):
        # ---- 1. continue from the latest archived checkpoint of each role (orchestration.py:146-211)
        for role in arch:
            ck = archive.sample_policy_from_archive(arch[role], role, "latest")
            if ck:
                trainer.load_state_dict(torch.load(ck, map_location=trainer.device, weights_only=True), roles=[role], optimizer=False)
        trainer.reset_optimizers()
        trainer.reset_episodes()
        # ---- 2. simultaneous training (agent_learning_utils.py:172-197)
        stats = trainer.train(trainer_cfg.timesteps)
        cop, thief = tc.cop_role_prefix, tc.thief_role_prefix
        ev = {cop: {}, thief: {}}
        chief_error = None
        if chief:
            try:
                # ---- 3. evaluation against archived opponents (:199-228)
                if league_eval:
                    ev = evaluate_agent_league(eval_env, evaluator, trainer, arch, tc, rng, log, frame_skip=trainer_cfg.frame_skip)
                else:
                    ev = {cop: evaluate_agent(eval_env, evaluator, trainer, cop, thief, arch[thief], tc, rng, log, tracked=tracked_eval, fused_eval=fused_eval, frame_skip=trainer_cfg.frame_skip),
                          thief: evaluate_agent(eval_env, evaluator, trainer, thief, cop, arch[cop], tc, rng, log, tracked=tracked_eval, fused_eval=fused_eval, frame_skip=trainer_cfg.frame_skip)}
                if position_stats is not None:
                    from ..render import write_heatmaps
                    write_heatmaps(out_dir / f"positions_iter_{it}", eval_env.position_tracker, getattr(eval_env, "maps", None) or load_preset(map_name, n_cops, n_thieves))
                    eval_env.position_tracker.clear()
                if baseline_env is not None:   # the trained policies against the scripted and the random opponents: absolute progress
                    b = evaluate_against_scripts(baseline_env, trainer, baseline_episodes, frame_skip=trainer_cfg.frame_skip, actor=baseline_actor)
                    baseline_log.append(dict({"iteration": it}, **b))
                    baselines_file.write_text(json.dumps(baseline_log, indent=1))
                    log("[self-play] baselines, cop win rate: " + ", ".join(f"{n} {r:.2f}" for n, r in zip(b["segments"], b["cop_win_rate"])))
                if navigator_env is not None:  # ... and against the privileged pursue / flee navigators: the distance to a map-aware opponent
                    b = evaluate_against_navigators(navigator_env, trainer, navigator_episodes, frame_skip=trainer_cfg.frame_skip, actor=navigator_actor)
                    navigator_log.append(dict({"iteration": it}, **b))
                    navigators_file.write_text(json.dumps(navigator_log, indent=1))
                    log("[self-play] navigators (privileged), cop win rate: " + ", ".join(f"{n} {r:.2f}" for n, r in zip(b["segments"], b["cop_win_rate"])))
                if separation_env is not None:  # ... and what the checkpoint catches from how far: the learned policies on both sides
                    b = evaluate_by_separation(separation_env, separation_actor, separation_eval, separation_episodes, source=trainer,
                                               frame_skip=trainer_cfg.frame_skip)
                    separation_log.append(dict({"iteration": it}, **b))
                    separation_file.write_text(json.dumps(separation_log, indent=1))
                    log("[self-play] cop win rate by initial separation: " + ", ".join(f"{lo}..{hi} {r:.2f}" for (lo, hi), r in zip(b["bands"], b["cop_win_rate"])))
                # ---- 4. joint checkpoint into both archives (orchestration.py:225-245)
                ck = out_dir / f"joint_iter_{it}_full_agent.pt"
                torch.save(trainer.state_dict(), ck)
                if it % tc.archive_save_interval == 0 or it == start + iterations - 1:
                    for role in arch:
                        archive.add_policy_to_archive(str(ck), arch[role], it, role)
                log(f"[self-play] iteration {it}: saved {ck.name}; evaluated {len(ev[cop])} thief and {len(ev[thief])} cop opponents"
                    + (f"; {world} ranks x {n_local} envs" if multi else "")
                    + ("; lr " + " ".join(f"{a}={stats[k]:.3g}" for a in trainer.agents for k in (f"lr/{a}",) if k in stats) if asked else "")
                    + (f"; training episodes{' of rank 0' if multi else ''} {stats['episodes']}, cop win rate {stats['cop_win_rate']:.3f}, mean length "
                       f"{stats['mean_episode_length']:.1f}" if episode_stats else ""))
                if episode_stats:
                    keys = ("episodes", "cop_win_rate", "mean_episode_length") + tuple(f"mean_return/{a}" for a in trainer.agents)
                    episode_log.append(dict({"iteration": it}, **{k: stats[k] for k in keys}))
                    stats_file.write_text(json.dumps(episode_log, indent=1))
            except Exception as exc:   # noqa: BLE001 -- handed to the other ranks below, then re-raised here
                if not multi:
                    raise
                chief_error = exc
        sync(ok=chief_error is None, what=f"while evaluating / saving iteration {it}")   # the other ranks read this iteration's archive entries in step 1 of the next
        if chief_error is not None:
            raise chief_error
        history.append({"iteration": it, "evaluations": ev, "stats": stats})
    return finish()


def planned_updates(iterations: int, trainer_cfg: TrainerConfig, cfg: RoleConfig) -> int:
    """The updates ``iterations`` calls of ``MAPPOTrainer.train(trainer_cfg.timesteps)`` make for a role configured by ``cfg``: one after
    every rollout of ``horizon`` ticks that ends at or beyond the role's ``learning_starts`` (at least 1)."""
    rollouts = -(-trainer_cfg.timesteps // trainer_cfg.horizon)
    first = max(1, -(-cfg.learning_starts // trainer_cfg.horizon))
    return max(1, iterations * max(0, rollouts - first + 1))


def launch_ranks(n: int, argv) -> int:
    """``--gpus N`` typed as a plain command: start N fresh rank processes of this module, one per GPU, through
    ``torch.distributed.run`` as a CHILD process (the bench.py pattern: never an exec, and this parent has not initialised the GPU)."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "as_cops_and_thieves_amd.selfplay.self_play", *argv]
    return subprocess.run(cmd, env=env).returncode


def group_timeout():
    """Collective timeout of the job's process group: the non-chief ranks wait in ``sync`` while rank 0 evaluates (2000-tick episodes
    against ``num_opponents_to_evaluate`` archived opponents per role) and writes checkpoints -- well beyond the backends' default of
    10 minutes on a slow disk or a long evaluation.  ``CAT_SELFPLAY_TIMEOUT_S`` (default two hours)."""
    import datetime
    return datetime.timedelta(seconds=float(os.environ.get("CAT_SELFPLAY_TIMEOUT_S", "7200")))


def init_ranks(gpus: int) -> str:
    """Inside a rank process (WORLD_SIZE set by the launcher): one GPU per rank and the RCCL group (``nccl`` IS RCCL on ROCm).
    ``CAT_SELFPLAY_REHEARSE=1``: the flow on a box with fewer GPUs than ranks -- ranks share devices, gloo carries the all-reduce
    (RCCL refuses two ranks on one device).  Returns the backend in use."""
    import torch.distributed as dist
    world, local = int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    if gpus != world:
        raise SystemExit(f"--gpus {gpus} inside a {world}-rank group: run the plain command, it starts its own ranks")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if os.environ.get("CAT_SELFPLAY_REHEARSE") == "1":
        torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
        dist.init_process_group("gloo", timeout=group_timeout())
        return "gloo (CAT_SELFPLAY_REHEARSE=1: ranks share devices)"
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local), timeout=group_timeout())
    probe = torch.ones(1, device=torch.device("cuda", local))
    dist.all_reduce(probe)
    if int(probe.item()) != world:
        raise RuntimeError(f"RCCL all-reduce of ones over {world} ranks returned {probe.item()}")
    return "nccl (RCCL)"


def parse_separation_bands(text: str) -> List[Tuple[int, int]]:
    """``LO:HI,LO:HI,...`` -> [(lo, hi), ...]; ValueError for anything but integers with 1 <= lo <= hi <= 65534."""
    from .curriculum import check_band
    bands = []
    for part in text.split(","):
        lo, sep, hi = part.strip().partition(":")
        if not sep or not lo.strip().isdigit() or not hi.strip().isdigit():
            raise ValueError(f"--separation-eval takes LO:HI,LO:HI,..., got {text!r}")
        bands.append(check_band(int(lo), int(hi)))
    return bands


def curriculum_options(args) -> dict:
    """The ``run_self_play`` arguments of the curriculum options of the command line; ValueError where they cannot apply."""
    out = {}
    if args.spawn_curriculum is None:
        if args.curriculum_adapt is not None:
            raise ValueError("--curriculum-adapt moves the band of --spawn-curriculum, which is not given")
    else:
        if args.gpus > 1:
            raise ValueError("--spawn-curriculum is a single-process option: it cannot be combined with --gpus > 1")
        out.update(spawn_curriculum=tuple(args.spawn_curriculum), curriculum_fraction=args.curriculum_fraction, curriculum_step=args.curriculum_step,
                   curriculum_max=args.curriculum_max)
        if args.curriculum_adapt is not None:
            out["curriculum_adapt"] = tuple(args.curriculum_adapt)
    if args.separation_eval is not None:
        if args.gpus > 1:
            raise ValueError("--separation-eval is a single-process option: it cannot be combined with --gpus > 1")
        out["separation_eval"] = parse_separation_bands(args.separation_eval)
        out["separation_episodes"] = args.separation_episodes
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="squarinth")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--timesteps", type=int, default=100_000, help="env ticks per iteration (reference: 100 000)")
    ap.add_argument("--out", type=Path, default=Path("lstm_policy_archive_self_play_new"))
    ap.add_argument("--strategy", default="pfsp", choices=["latest", "random", "pfsp"])
    ap.add_argument("--eval-envs", type=int, default=None)
    ap.add_argument("--max-step-count", type=int, default=2000, help="episode cap (self_play_driver.py:34 passes 2000)")
    ap.add_argument("--horizon", type=int, default=None, help="rollout ticks per update (TrainerConfig default: 128)")
    ap.add_argument("--cops", type=int, default=None)
    ap.add_argument("--thieves", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--per-role-configs", action="store_true", help="CFG_AGENT_COP / CFG_AGENT_THIEF (mappo_config.py:19-39) instead of CFG_AGENT for both")
    ap.add_argument("--random-timesteps", type=int, default=None, help="override of the role configs' random_timesteps (mappo_config.py:9: 10000)")
    ap.add_argument("--learning-starts", type=int, default=None, help="override of learning_starts (mappo_config.py:10: 15000)")
    ap.add_argument("--freeze-duration", type=int, default=None, help="override of CFG_TRAINER's policy / opponent freeze durations (15000)")
    ap.add_argument("--non-recurrent", action="store_true", help="the reference's non-recurrent Policy / Value pair (policy_net.py, value_net.py; "
                    "model_utils.py:45-77) instead of the LSTM pair its drivers use")
    ap.add_argument("--query-order", default="index", choices=["index", "chipmunk"],
                    help="visiting order of the walls in segment queries: index order (default) or Chipmunk's static tree (DESIGN.md D2)")
    ap.add_argument("--tracked-eval", action="store_true", help="evaluate through evaluate_agents_tracked: episode book-keeping on the device, "
                    "the host polls every 32 ticks instead of every tick")
    ap.add_argument("--fused-eval", action="store_true", help="evaluate through a PolicyActor (policy blocks only; on a GPU one launch per act tick) "
                    "instead of a second trainer")
    ap.add_argument("--league-eval", action="store_true", help="evaluate both roles against all their drawn opponents in one pass through a LeagueActor "
                    "(one act launch per tick for every match-up); not with --tracked-eval")
    ap.add_argument("--baseline-eval", action="store_true", help="after every iteration play the trained policies against the scripted chase / evade "
                    "opponents and against random ones in one pass (selfplay/scripted.py) and append the result to baselines.json")
    ap.add_argument("--baseline-episodes", type=int, default=64, help="--baseline-eval: episodes per match-up (four match-ups share one env)")
    ap.add_argument("--navigator-eval", action="store_true", help="after every iteration play the trained policies against the PRIVILEGED pursue / flee "
                    "navigators (selfplay/navigators.py: they read true positions and the map) and append the result to navigators.json")
    ap.add_argument("--navigator-episodes", type=int, default=64, help="--navigator-eval: episodes per match-up (the match-ups run one after another)")
    ap.add_argument("--episode-stats", action="store_true", help="account the training episodes on the device: win rate and mean length in "
                    "every iteration's log line, episode_stats.json in --out (with --gpus N: of rank 0's shard)")
    ap.add_argument("--role-training", action="store_true", help="the reference's role-training mode (fictitious play): per iteration a cop phase, then a "
                    "thief phase, each against archived opponents drawn by --strategy, all at once on segments of the env batch; not with --tracked-eval or --gpus > 1")
    ap.add_argument("--training-opponents", type=int, default=8, help="--role-training: archived opponents a phase trains against at once (1..32)")
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel ranks, one per GPU: --envs is the TOTAL, sharded across them")
    ap.add_argument("--frame-skip", type=int, default=1, help="env ticks per decision (action repeat) in training and in the evaluations; above 1 "
                    "--timesteps, --horizon and the schedule options count decisions")
    ap.add_argument("--position-stats", type=int, default=None, metavar="CELL", help="occupancy / exposure / spawn heatmaps of every iteration's evaluation "
                    "on a grid of CELL x CELL pixels, written to positions_iter_N/ in --out")
    ap.add_argument("--fused-collect", action="store_true", help="collect the training rollouts through the one-launch fused act kernel "
                    "(TrainerConfig.fused_collect: a GPU, bf16, the recurrent pair, 64 or 90 rays)")
    ap.add_argument("--lr-schedule", choices=("constant", "linear", "kl_adaptive"), default="constant", help="learning-rate schedule of both roles "
                    "(RoleConfig.lr_schedule): linear to --lr-final over the run's updates, or KL-adaptive per agent (skrl's KLAdaptiveLR rule); "
                    "constant in the reference")
    ap.add_argument("--lr-final", type=float, default=None, help="end value of --lr-schedule linear")
    ap.add_argument("--lr-kl-target", type=float, default=None, help="KL target of --lr-schedule kl_adaptive (RoleConfig default: 0.008)")
    ap.add_argument("--entropy-final", type=float, default=None, help="anneal the entropy scale linearly to this value over the run's updates")
    ap.add_argument("--clip-final", type=float, default=None, help="anneal the ratio clip linearly to this value over the run's updates")
    ap.add_argument("--value-norm", action="store_true", help="train the critics on returns normalised by running per-agent moments "
                    "(TrainerConfig.value_norm; off in the reference)")
    ap.add_argument("--geodesic-shaping", type=float, default=0.0, metavar="W", help="geodesic potential-based reward shaping of the learners with "
                    "scale W per hop (TrainerConfig.geodesic_shaping; 0 = off, as the reference trains)")
    ap.add_argument("--shaping-scale-thief", type=float, default=None, metavar="W", help="the thieves' shaping scale (default: that of the cops)")
    ap.add_argument("--shaping-cap", type=int, default=None, metavar="H", help="hop counts above H count as H (default 64)")
    ap.add_argument("--spawn-curriculum", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="a geodesic start-state curriculum: a training slot "
                    "whose episode ended respawns with every cop LO .. HI shortest-path hops from a thief (TrainerConfig.spawn_curriculum; the "
                    "evaluation envs keep the map's own spawn); not with --gpus > 1")
    ap.add_argument("--curriculum-fraction", type=float, default=1.0, metavar="F", help="the share of the training slots that takes the band (the first ones)")
    ap.add_argument("--curriculum-adapt", type=float, nargs=2, default=None, metavar=("LOW", "HIGH"), help="move HI with the cops' win rate between "
                    "updates: above HIGH it rises, below LOW it falls")
    ap.add_argument("--curriculum-step", type=int, default=1, metavar="S", help="--curriculum-adapt: hops per move")
    ap.add_argument("--curriculum-max", type=int, default=64, metavar="H", help="--curriculum-adapt: the largest HI")
    ap.add_argument("--separation-eval", default=None, metavar="LO:HI,LO:HI,...", help="after every iteration the cops' win rate as a function of the "
                    "initial geodesic separation: one pass over an env cut into one segment per band, appended to separation.json")
    ap.add_argument("--separation-episodes", type=int, default=64, help="--separation-eval: episodes (slots) per band")
    return ap


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    curriculum = curriculum_options(args)
    if args.role_training and args.gpus > 1:
        sys.exit("--role-training is a single-process mode: it cannot be combined with --gpus > 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv)))          # plain command: start the ranks ourselves
    backend = None
    if args.gpus > 1:
        backend = init_ranks(args.gpus)
    tc = TrainingConfig(policy_sample_strategy=args.strategy, training_timesteps_per_role_training=args.timesteps,
                        num_training_opponents=args.training_opponents)
    over = {"horizon": args.horizon} if args.horizon else {}
    if args.frame_skip != 1:
        over["frame_skip"] = args.frame_skip
    if args.non_recurrent:
        over["recurrent"] = False
    if args.freeze_duration is not None:
        over.update(policy_freeze_duration=args.freeze_duration, opponent_freeze_duration=args.freeze_duration)
    tcfg = TrainerConfig(timesteps=args.timesteps, **over)
    from .mappo import CFG_AGENT_COP, CFG_AGENT_THIEF
    role_cfg = {"cop": CFG_AGENT_COP, "thief": CFG_AGENT_THIEF} if args.per_role_configs else {"cop": CFG_AGENT, "thief": CFG_AGENT}
    sched = {k: v for k, v in (("random_timesteps", args.random_timesteps), ("learning_starts", args.learning_starts)) if v is not None}
    role_cfg = {r: dataclasses.replace(c, **sched) for r, c in role_cfg.items()}
    rank = int(os.environ.get("RANK", "0"))
    res = run_self_play(args.map, args.envs, args.out, iterations=args.iterations, training=tc, trainer_cfg=tcfg, role_cfg=role_cfg,
                        num_rays=args.rays, n_cops=args.cops, n_thieves=args.thieves, max_step_count=args.max_step_count,
                        eval_envs=args.eval_envs, seed=args.seed, log=print if rank == 0 else (lambda *a, **k: None),
                        query_order=args.query_order, tracked_eval=args.tracked_eval, episode_stats=args.episode_stats, fused_eval=args.fused_eval,
                        league_eval=args.league_eval, **({"role_training": True} if args.role_training else {}),
                        **({"fused_collect": True} if args.fused_collect else {}), **({"value_norm": True} if args.value_norm else {}),
                        **({"geodesic_shaping": args.geodesic_shaping, "shaping_scale_thief": args.shaping_scale_thief, "shaping_cap": args.shaping_cap}
                           if (args.geodesic_shaping or args.shaping_scale_thief) else {}),
                        **({"position_stats": args.position_stats} if args.position_stats is not None else {}), **curriculum,
                        **({"baseline_eval": True, "baseline_episodes": args.baseline_episodes} if args.baseline_eval else {}),
                        **({"navigator_eval": True, "navigator_episodes": args.navigator_episodes} if args.navigator_eval else {}),
                        **{k: v for k, v in (("lr_schedule", args.lr_schedule), ("lr_final", args.lr_final), ("lr_kl_target", args.lr_kl_target),
                                             ("entropy_final", args.entropy_final), ("ratio_clip_final", args.clip_final))
                           if v not in (None, "constant")})
    if backend:
        import torch.distributed as dist
        print(f"[self-play] rank {res['rank']}/{res['world']}: {res['envs_local']} envs from global id {res['env_id_offset']}, all-reduce over "
              f"{backend}, parameters {res['param_digest'][:16]}", flush=True)
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
