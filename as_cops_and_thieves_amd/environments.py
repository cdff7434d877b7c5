"""Environment classes: the drop-in boundary of the hot path.

``BaseEnv`` / ``SimpleEnv`` mirror reference ``src/environments/base_env.py`` and
``simple_env.py`` (PettingZoo ``ParallelEnv`` surface, one env, per-agent dicts of NumPy arrays),
so a ``driver.py``-style loop, skrl's PettingZoo wrapper and ``evaluate_agents``
(``src/utils/eval_pfsp_agents.py:25-49``) run against them unchanged — except that the tick is
computed by the HIP kernels behind ``libcat_sim.so`` instead of Pymunk.  ``VecCopsEnv`` is the
batched form of the same surface: same keys, values are torch tensors with a leading ``num_envs``
axis, finished episodes auto-reset on device.

``BaseEnv`` subclasses ``pettingzoo.ParallelEnv`` when pettingzoo is importable (it is not installable in the build
container, where the class is duck-typed to the attributes its wrappers use; ``tests/test_gpu_boundary_double.py``
drives exactly those).  There is no CPU path: constructing an env without the built extension or without a GPU raises.
"""
from __future__ import annotations

import itertools
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import spaces
from .agents import Cop, Entity, Thief
from .config import SimConfig
from .constants import DEFAULT_SENSOR, PhysicalParams, load_physical_params
from .maps import CompiledMap, Map
from .observation_spaces import (_init_shared_observation_space,
                                 get_nested_agent_observation_spaces as _nested_spaces)
from ._native import MAX_ROLLOUT_TICKS as _MAX_REPEAT
from .sim import CatSim

WINNER_NAMES = {-1: None, 0: "cop", 1: "thief"}

try:  # pragma: no cover - depends on the installation
    from pettingzoo import ParallelEnv as _ParallelEnvBase  # type: ignore
    HAVE_PETTINGZOO = True
except ModuleNotFoundError:
    _ParallelEnvBase = object
    HAVE_PETTINGZOO = False


def _physical_from_cwd() -> PhysicalParams:
    """The reference reads ``pyproject.toml [tool.physical-params]`` from the CWD
    (``src/utils/toml_utils.py:40-46``); honour such a file when present, else the defaults."""
    p = Path("pyproject.toml")
    if p.exists():
        try:
            return load_physical_params(p)
        except (KeyError, OSError, ValueError):
            pass
    return load_physical_params(None)


QUERY_ORDERS = ("index", "chipmunk")


def gate_mode(bbtree_gate: bool, query_order: str) -> int:
    """``SimConfig.bbtree_gate`` for the env options: 0 no gate, 1 the gate with the walls in index order (the default), 2 the gate with the walls in
    the order of Chipmunk's static tree (``query_order="chipmunk"``).  The tree order is an order of the GATED query, so it needs the gate."""
    if query_order not in QUERY_ORDERS:
        raise ValueError(f"query_order must be one of {QUERY_ORDERS}, not {query_order!r}")
    if query_order == "chipmunk":
        if not bbtree_gate:
            raise ValueError('query_order="chipmunk" orders the gated segment query: it needs bbtree_gate=True')
        return 2
    return int(bool(bbtree_gate))


class BaseEnv(_ParallelEnvBase):
    """Single-env PettingZoo ``ParallelEnv`` surface (reference ``BaseEnv(ParallelEnv)``, base_env.py:30-554)."""

    metadata = {"render_modes": ["human", "rgb_array"], "name": "cops_and_thieves_amd"}

    def __init__(self, map: Map, map_image: Optional[Path] = None, render_mode: Optional[str] = None,
                 max_step_count: int = 400, time_step: float = 1 / 15.0, *,
                 num_rays: int = DEFAULT_SENSOR.num_rays, device=None, seed: int = 1,
                 physical: Optional[PhysicalParams] = None, bbtree_gate: bool = True, query_order: str = "index"):
        gate = gate_mode(bbtree_gate, query_order)   # (before anything touches a device)
        assert render_mode is None or render_mode in self.metadata["render_modes"]  # base_env.py:117
        self.map, self.map_image = map, map_image
        self.width, self.height = self.map.window_dimensions
        self.step_count = 0
        self.max_step_count, self.time_step = max_step_count, time_step
        self.render_mode = render_mode
        physical = physical or _physical_from_cwd()
        self.cop_category = physical.pymunk_cop_category
        self.thief_category = physical.pymunk_thief_category
        self._termination_radius = physical.termination_radius

        self._cfg = SimConfig.from_params(
            physical=physical, n_envs=1, n_cops=map.cops_count, n_thieves=map.thieves_count,
            max_step_count=max_step_count, dt=time_step, seed=seed, bbtree_gate=gate)
        self._cfg.n_rays = num_rays
        self._compiled: CompiledMap = map.compile(self._cfg.wall_radius)
        self._sim = CatSim(self._cfg, [self._compiled], device=device)

        group_counter = itertools.count(1)                              # base_env.py:90-92
        A = self._cfg.n_agents
        self.cops: List[Cop] = [
            Cop(self, i, f"cop_{i}", next(group_counter), self.cop_category, num_rays, self._cfg.ray_length, physical)
            for i in range(map.cops_count)]
        self.thieves: List[Thief] = [
            Thief(self, map.cops_count + j, f"thief_{j}", next(group_counter), self.thief_category, num_rays,
                  self._cfg.ray_length, physical)
            for j in range(map.thieves_count)]
        everyone: List[Entity] = self.cops + self.thieves
        assert len(everyone) == A
        self.possible_agents = [a.get_id() for a in everyone]           # base_env.py:96
        self.agents: List[str] = []
        self.agent_name_mapping = {a.get_id(): a for a in everyone}
        self.observation_spaces = {a.get_id(): a.observation_space for a in everyone}
        self.action_spaces = {a.get_id(): a.action_space for a in everyone}
        shared = _init_shared_observation_space(map=self.map, cops=self.cops, thieves=self.thieves)
        self.shared_observation_spaces = shared                         # replaced by VALUES after reset()
        self._shared_observation_spaces = shared
        self.state_space = shared
        self._state_cache: Dict[str, np.ndarray] = {}

    # ---- PettingZoo conveniences -------------------------------------------------------
    @property
    def unwrapped(self):
        return self

    @property
    def num_agents(self) -> int:
        return len(self.agents)

    @property
    def max_num_agents(self) -> int:
        return len(self.possible_agents)

    def observation_space(self, agent: str):
        return self.agent_name_mapping[agent].observation_space

    def action_space(self, agent: str):
        return self.agent_name_mapping[agent].action_space

    def get_base_observation_space_structure(self):
        return self._shared_observation_spaces

    def get_nested_agent_observation_spaces(self):
        return _nested_spaces(self._shared_observation_spaces)

    # ---- helpers ---------------------------------------------------------------------------
    def _host_state(self, name: str) -> np.ndarray:
        return self._sim.get_state()[name].cpu().numpy()

    def _observations_from_outputs(self) -> Dict[str, dict]:
        out = self._sim.out
        torch.cuda.current_stream(self._sim.device).synchronize()
        dist = out["obs_distance"][0].cpu().numpy()                     # [A,R] float16
        typ = out["obs_type"][0].cpu().numpy()
        obs = {aid: {"distance": dist[i].copy(), "object_type": typ[i].copy()}
               for i, aid in enumerate(self.possible_agents)}
        # get_shared_observations (observation_spaces.py:98-129): the two aggregate arrays and the
        # team positions are shared (aliased) by all members of a team
        sd = out["shared_distance"][0].cpu().numpy()
        st = out["shared_type"][0].cpu().numpy()
        tp = out["team_positions"][0].cpu().numpy()
        nc = self.map.cops_count
        shared = {}
        for team, members, positions in ((0, self.cops, tp[:nc]), (1, self.thieves, tp[nc:])):
            if not members:
                continue
            team_obj, team_dist, team_pos = st[team].copy(), sd[team].copy(), positions.copy()
            for agent in members:
                aid = agent.get_id()
                shared[aid] = {"own_obj_types": obs[aid]["object_type"], "own_distances": obs[aid]["distance"],
                               "object_type_shared": team_obj, "distance_shared": team_dist,
                               "team_positions": team_pos}
        self.shared_observation_spaces = shared
        return obs

    # ---- reset / step ------------------------------------------------------------------------
    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        """base_env.py:286-352.  ``options={"positions": [[x, y], ...]}`` (cops first) injects the
        spawn positions instead of sampling them (build-side extension used by parity tests)."""
        if seed is not None:
            self._sim.set_seed(seed)
        self.agents = self.possible_agents[:]
        for agent_id in self.agents:                                    # base_env.py:323-332 warnings
            regions = self.map.agent_spawn_regions.get(agent_id)
            if agent_id not in self.map.agent_spawn_regions:
                print(f"Warning: No spawn regions defined in map for agent {agent_id}. Using default reset "
                      f"(current position or initial).")
            elif not regions:
                print(f"Warning: Agent {agent_id} has an empty list of spawn regions. Using default reset "
                      f"(current position or initial).")
        positions = None
        if options and options.get("positions") is not None:
            positions = torch.as_tensor(np.asarray(options["positions"], dtype=np.float64)).reshape(1, -1, 2)
        self._sim.reset(positions=positions)
        observations = self._observations_from_outputs()
        infos = {agent_id: {} for agent_id in self.agents}
        self.step_count = 0
        return observations, infos

    def step(self, action: dict):
        """base_env.py:354-413."""
        self.step_count += 1
        if not action:                                                  # :374-376
            self.agents = []
            sc = self._sim.get_state()["step_count"]
            self._sim.set_state(step_count=sc + 1)
            return {}, {}, {}, {}, {}
        if not self.agents:
            # the reference unpacks an empty result list here (base_env.py:384-386)
            sc = self._sim.get_state()["step_count"]
            self._sim.set_state(step_count=sc + 1)
            raise ValueError("not enough values to unpack (expected 5, got 0)")
        acts = np.empty((1, len(self.possible_agents)), dtype=np.int32)
        for i, agent in enumerate(self.agents):
            a = action[agent]                                           # KeyError for a missing agent
            a = int(a.item()) if hasattr(a, "item") else int(a)
            if a not in (0, 1, 2, 3):
                raise TypeError(f"invalid action {a!r} for agent {agent}: expected one of 0..3")
            acts[0, i] = a
        self._sim.step(torch.from_numpy(acts))
        observations = self._observations_from_outputs()
        out = self._sim.out
        rew = out["reward"][0].cpu().numpy()
        terminated = bool(out["terminated"][0].item())
        truncated = bool(out["truncated"][0].item())
        winner = WINNER_NAMES[int(out["winner"][0].item())]
        rewards = {a: float(rew[i]) for i, a in enumerate(self.agents)}
        terminations = {a: terminated for a in self.agents}             # entity.py:146
        truncations = {a: truncated for a in self.agents}               # base_env.py:397
        infos = {a: {"winner": winner} for a in self.agents}            # :410-411
        if terminated:
            self.agents = []                                            # :401-402
        return observations, rewards, terminations, truncations, infos

    def state(self) -> dict:
        return self.shared_observation_spaces                           # base_env.py:415-425

    def render(self):
        if self.render_mode == "rgb_array":
            from .render import render_rgb_array
            st = self._sim.get_state()
            return render_rgb_array(self._compiled, st["pos"][0].cpu().numpy(), self.map.cops_count,
                                    self._cfg.agent_radius)
        return None

    def close(self) -> None:
        self._sim.close()

    def _get_info(self) -> dict:
        return {"step_count": self.step_count, "thief_count": len(self.thieves), "cop_count": len(self.cops)}


class SimpleEnv(BaseEnv):
    """reference ``SimpleEnv`` (simple_env.py:6-58): dt = 1/60, render_mode "rgb_array"."""

    def __init__(self, map: Map, render_mode: str = "rgb_array", map_image: Optional[Path] = None,
                 max_step_count: int = 400, time_step: float = 1 / 60.0, query_order: str = "index", **kw):
        super().__init__(map=map, map_image=map_image, render_mode=render_mode,
                         max_step_count=max_step_count, time_step=time_step, query_order=query_order, **kw)

    def _get_info(self) -> dict:
        info = super()._get_info()
        pos = self._host_state("pos")[0]
        nc = self.map.cops_count
        info.update({"environment_type": "SimpleEnv",
                     "thief_positions": [tuple(int(v) for v in p) for p in pos[nc:]],
                     "cop_positions": [tuple(int(v) for v in p) for p in pos[:nc]]})
        return info


def raw_env(map: Map, render_mode: str = "rgb_array", **kw):
    """reference ``raw_env`` (base_env.py:555-569): the single env wrapped for PettingZoo's AEC API with
    ``pettingzoo.utils.conversions.parallel_to_aec``.  Needs pettingzoo (the conversion is its code, not restated here): without
    it an ImportError says so.  ``kw`` goes to ``BaseEnv`` (device, num_rays, ...)."""
    try:
        from pettingzoo.utils.conversions import parallel_to_aec
    except ImportError as exc:
        raise ImportError("raw_env() returns pettingzoo's AEC wrapper of BaseEnv and needs the pettingzoo package "
                          "(BaseEnv / SimpleEnv / VecCopsEnv work without it)") from exc
    return parallel_to_aec(BaseEnv(map=map, render_mode=render_mode, **kw))


def check_repeat(repeat, what: str = "repeat") -> int:
    """A frame-skip count: an integer >= 1 (and within one resident launch), else ValueError."""
    if isinstance(repeat, bool) or not isinstance(repeat, (int, np.integer)) or not 1 <= int(repeat) <= _MAX_REPEAT:
        raise ValueError(f"{what} must be an integer in 1..{_MAX_REPEAT}, got {repeat!r}")
    return int(repeat)


class VecCopsEnv:
    """Batched env: ``num_envs`` independent envs advanced in lock-step on one GPU.

    Same agent ids, spaces and dict keys as ``BaseEnv``; every value is a torch tensor on the
    device with a leading ``num_envs`` axis (zero-copy views of the buffers the kernels write).
    After a terminal tick the env slot is reset on device (``auto_reset``), and the observation
    returned for that slot is the first observation of the new episode; ``infos`` carries the
    per-slot ``winner`` (int8: -1 none, 0 cop, 1 thief), ``terminated`` and ``truncated`` flags of
    the tick that just ended.

    ``track_episodes=True`` (needs ``auto_reset``): an ``episodes.EpisodeTracker`` on the device adds the ticks of ``step``,
    ``step_raw`` and ``rollout_random`` up into episodes -- returns, lengths, outcomes (``episode_stats()``); an explicit
    ``reset`` abandons the episodes it cuts short.  Off by default: nothing is launched or stored.

    Frame skip (action repeat): ``step(actions, repeat=k)`` / ``step_raw(actions, repeat=k)`` with ``k > 1`` play up to ``k`` env ticks
    per slot with the actions held, in one resident launch (``CatSim.step_repeat``).  A slot stops at the tick that ends its episode
    (the new episode is reset but not stepped with the stale action); rewards are the fp32 sums over the ticks played, observations
    and flags those of the slot's last played tick, and ``infos["ticks"]`` / ``out["ticks"]`` the ticks played.  ``frame_skip=k`` in
    the constructor sets the default ``repeat``.  ``repeat == 1`` is the one-tick path, unchanged.  With ``track_episodes`` the tracker
    is given each row's tick count, so lengths, the histogram and the outcomes stay in env ticks; a return is the f64 sum of the fp32
    window sums (``EpisodeTracker.update``).  ``out["ticks"]`` is written by repeat calls only: after a later one-tick step it still
    holds the last repeat call's counts.

    ``track_positions=CELL`` (needs ``auto_reset``): a ``positions.PositionTracker`` on the device adds the rows of ``step``, ``step_raw``
    (one row per call, whatever ``repeat`` is) and ``rollout_random`` into occupancy / exposure / spawn maps on a grid of CELL x CELL pixels
    over the batch's largest map window (``position_stats()``, ``position_tracker``); ``position_exposure=False`` leaves ``obs_type`` unread
    and the SEEN plane zero; ``position_groups`` is the tracker's number of groups (``PositionTracker.set_groups``; every slot starts in
    group 0).  An explicit ``reset`` feeds nothing.  Off by default: no buffer, no launch.

    ``final_positions=True``: where episodes END.  Under auto-reset a terminal row's ``team_positions`` is already the spawn point of the next
    episode; with this option the env owns a float16 ``[N, A, 2]`` buffer, bound to the env core for its whole life
    (``CatSim.bind_final_positions``), and ``step`` / ``step_raw`` (``repeat=k`` included) / ``rollout_random`` expose it as
    ``infos["final_positions"]`` / ``out["final_positions"]`` (a view of the buffer, not a copy).  Where ``terminated`` is set the row holds
    the tick-start positions of the tick that ended the episode -- what the termination check read.  EVERY OTHER ROW IS NOT WRITTEN: it keeps
    the positions of that slot's last episode end, and NaN (``0x7E00``) before the slot's first.  Mask with ``terminated``.  The buffer's
    address never changes, so a HIP graph captured over the env's ticks keeps filling it.  With ``track_positions`` the tracker also keeps the
    capture / timeout maps (``PositionTracker(final_positions=True)``).  Off by default: no buffer, no bind, nothing changes.
    """

    metadata = BaseEnv.metadata
    TRACKED_ROLLOUT_BYTES = 64 << 20    # rollout_random with tracking: most bytes of reward / flag rows kept per resident launch

    def __init__(self, maps, num_envs: int, *, slot_map_ids: Optional[Sequence[int]] = None,
                 num_rays: int = 64, max_step_count: int = 400, time_step: float = 1 / 60.0,
                 auto_reset: bool = True, device=None, seed: int = 1, env_id_offset: int = 0,
                 physical: Optional[PhysicalParams] = None, bbtree_gate: bool = True, query_order: str = "index",
                 track_episodes: bool = False, frame_skip: int = 1, track_positions: Optional[int] = None,
                 position_exposure: bool = True, position_groups: int = 1, final_positions: bool = False):
        gate = gate_mode(bbtree_gate, query_order)   # (before anything touches a device)
        self.frame_skip = check_repeat(frame_skip, "frame_skip")
        if track_episodes and not auto_reset:
            raise ValueError("track_episodes=True needs auto_reset=True: the accounting restarts a slot's episode at its terminal tick")
        if track_positions is not None:
            if not auto_reset:
                raise ValueError("track_positions needs auto_reset=True: a terminal row counts as the spawn of the slot's next episode")
            if isinstance(track_positions, bool) or not isinstance(track_positions, (int, np.integer)) or track_positions < 1:
                raise ValueError(f"track_positions is the cell size in pixels, an integer >= 1, got {track_positions!r}")
        self.maps: List[Map] = list(maps) if isinstance(maps, (list, tuple)) else [maps]
        m0 = self.maps[0]
        for m in self.maps[1:]:
            if (m.cops_count, m.thieves_count) != (m0.cops_count, m0.thieves_count):
                raise ValueError("all maps of a batch must share one roster")
        physical = physical or _physical_from_cwd()
        self.num_envs, self.auto_reset = num_envs, auto_reset
        self._cfg = SimConfig.from_params(
            physical=physical, n_envs=num_envs, n_cops=m0.cops_count, n_thieves=m0.thieves_count,
            max_step_count=max_step_count, dt=time_step, seed=seed, env_id_offset=env_id_offset,
            bbtree_gate=gate)
        self._cfg.n_rays = num_rays
        self._compiled = [m.compile(self._cfg.wall_radius) for m in self.maps]
        self._sim = CatSim(self._cfg, self._compiled, slot_map_ids, device=device)
        self.device = self._sim.device
        self.slot_map_ids = np.zeros(num_envs, dtype=np.int32) if slot_map_ids is None else \
            np.array(slot_map_ids, dtype=np.int32).reshape(num_envs)   # (cat_create has checked them)
        self._render_scene = None
        self.possible_agents = [f"cop_{i}" for i in range(m0.cops_count)] + \
                               [f"thief_{j}" for j in range(m0.thieves_count)]
        self.agents = self.possible_agents[:]
        group = itertools.count(1)
        self.cops = [Cop(self, i, f"cop_{i}", next(group), physical.pymunk_cop_category, num_rays,
                         self._cfg.ray_length, physical) for i in range(m0.cops_count)]
        self.thieves = [Thief(self, m0.cops_count + j, f"thief_{j}", next(group), physical.pymunk_thief_category,
                              num_rays, self._cfg.ray_length, physical) for j in range(m0.thieves_count)]
        everyone = self.cops + self.thieves
        self.agent_name_mapping = {a.get_id(): a for a in everyone}
        self.observation_spaces = {a.get_id(): a.observation_space for a in everyone}
        self.action_spaces = {a.get_id(): a.action_space for a in everyone}
        self._shared_observation_spaces = _init_shared_observation_space(m0, self.cops, self.thieves)
        self.state_space = self._shared_observation_spaces
        self.max_step_count, self.time_step = max_step_count, time_step
        self._actions = torch.zeros((num_envs, len(everyone)), dtype=torch.int32, device=self.device)
        self._spawner = None            # set_spawner: a geodesic start-state curriculum (selfplay/curriculum.py)
        self._tracker = None
        if track_episodes:
            from .episodes import EpisodeTracker
            self._tracker = EpisodeTracker(num_envs, self.possible_agents, max_step_count, self.device)
        self._final_pos = self._final_rows = None
        if final_positions:
            from .sim import FINAL_POS_NAN
            self._final_pos = torch.full((num_envs, len(everyone), 2), FINAL_POS_NAN, dtype=torch.int16, device=self.device).view(torch.float16)
            self._sim.bind_final_positions(self._final_pos)
            self._sim.out["final_positions"] = self._final_pos      # (not a field of cat_outputs: the sim's launches never look it up)
        if track_episodes or track_positions is not None:
            self._tracked_rows: Dict[str, torch.Tensor] = {}
        self._positions, self._exposure = None, bool(position_exposure)
        if track_positions is not None:
            from .positions import PositionTracker
            window = (max(int(c.window[0]) for c in self._compiled), max(int(c.window[1]) for c in self._compiled))
            self._positions = PositionTracker(num_envs, self.possible_agents, m0.cops_count, window, int(track_positions), int(position_groups), self.device,
                                              final_positions=bool(final_positions))

    # episode accounting
    @property
    def episode_tracker(self):
        """The ``EpisodeTracker`` that ``step`` / ``step_raw`` / ``rollout_random`` feed."""
        if self._tracker is None:
            raise RuntimeError("this VecCopsEnv was built without track_episodes=True: it keeps no episode statistics")
        return self._tracker

    def episode_stats(self, clear: bool = False, segments=None) -> dict:
        """``EpisodeTracker.summary()`` of the episodes finished since the last clear (one synchronisation).  ``segments``: S + 1 row bounds
        of contiguous slot segments (0 first, ``num_envs`` last, strictly increasing) -- the dict then carries ``"segments"``, the
        ``EpisodeTracker.segment_summary`` of those (one more launch and copy)."""
        segs = None if segments is None else self.episode_tracker.segment_summary(segments)     # bad bounds raise before anything is read
        stats = self.episode_tracker.summary()
        if segs is not None:
            stats["segments"] = segs
        if clear:
            self._tracker.clear()
        return stats

    @property
    def position_tracker(self):
        """The ``PositionTracker`` that ``step`` / ``step_raw`` / ``rollout_random`` feed."""
        if self._positions is None:
            raise RuntimeError("this VecCopsEnv was built without track_positions=CELL: it keeps no position statistics")
        return self._positions

    def position_stats(self, clear: bool = False) -> list:
        """``PositionTracker.summary()`` of the rows counted since the last clear (one synchronisation)."""
        stats = self.position_tracker.summary()
        if clear:
            self._positions.clear()
        return stats

    def _track(self, out, ticks=None) -> None:
        if self._tracker is not None:
            self._tracker.update(out["reward"], out["terminated"], out["truncated"], out["winner"], ticks=ticks)
        if self._positions is not None:     # a frame-skip row counts once, at the window's last position
            ends = {"final_positions": out["final_positions"], "truncated": out["truncated"]} if "final_positions" in out else {}
            self._positions.update(out["team_positions"], out["terminated"], out["obs_type"] if self._exposure else None, **ends)

    def _repeat(self, repeat) -> int:
        """The ``repeat`` argument of ``step`` / ``step_raw``, checked: None is the constructor's ``frame_skip``."""
        return self.frame_skip if repeat is None else check_repeat(repeat)

    def set_spawner(self, spawner=None) -> None:
        """Attach a ``selfplay.curriculum.GeodesicSpawner`` built over this env (None, the default, detaches it): ``step`` / ``step_raw``
        (``repeat=k`` included) then respawn every slot whose episode just ended by the spawner's rule, right after the tick's launch and
        before anything reads the new episode's first state -- the position tracker's SPAWN plane, ``observations()``, a
        ``GeodesicShaper`` and the actors all see the start state the episode really has -- and ``reset`` without explicit positions
        places its slots the same way.  ``out["ticks"]``, the rewards, the flags, ``winner`` and ``final_positions`` stay the terminal
        tick's.  Slots the rule cannot serve, or whose band is off, keep the map's own spawn.  A respawned slot's ``reset_count``
        advances twice per episode, which shifts the slot's Philox spawn stream and nothing else.  ``rollout_random`` raises ValueError
        while a spawner is attached: the resident launch cannot respawn between its ticks.  Off: one ``is None`` test per step on the
        host, the launches are unchanged."""
        if spawner is not None:
            if not self.auto_reset:
                raise ValueError("a spawner needs auto_reset=True: it re-places the slots the tick has just reset")
            if getattr(spawner, "N", None) != self.num_envs or getattr(spawner, "A", None) != len(self.possible_agents) or \
                    torch.device(spawner.device) != torch.device(self.device):
                raise ValueError(f"the spawner must be built over this env ({self.num_envs} envs, {len(self.possible_agents)} agents, {self.device})")
        self._spawner = spawner

    def _spawn_reset(self, mask, positions) -> None:
        """What a spawner calls: one masked ``cat_reset`` launch with injected positions (no allocation, no synchronisation)."""
        self._sim.reset(mask=mask, positions=positions)

    def _step_sim(self, acts, repeat: int):
        if repeat == 1:
            out = self._sim.step_fused(acts, auto_reset=self.auto_reset)
            if self._spawner is not None:
                self._spawner.respawn(out)
            self._track(out)
            return out
        out = self._sim.step_repeat(acts, repeat, auto_reset=self.auto_reset)
        if self._spawner is not None:
            self._spawner.respawn(out)
        self._track(out, out["ticks"])      # a row of a repeat call stands for ticks[n] env ticks of slot n
        return out

    # spaces
    def observation_space(self, agent: str):
        return self.observation_spaces[agent]

    def action_space(self, agent: str):
        return self.action_spaces[agent]

    def get_base_observation_space_structure(self):
        return self._shared_observation_spaces

    def get_nested_agent_observation_spaces(self):
        return _nested_spaces(self._shared_observation_spaces)

    def _host_state(self, name: str) -> np.ndarray:
        return self._sim.get_state()[name].cpu().numpy()

    def _obs(self) -> Dict[str, Dict[str, torch.Tensor]]:
        o = self._sim.out
        return {aid: {"distance": o["obs_distance"][:, i], "object_type": o["obs_type"][:, i]}
                for i, aid in enumerate(self.possible_agents)}

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        if seed is not None:
            self._sim.set_seed(seed)
        positions = None if not options else options.get("positions")
        mask = None if not options else options.get("mask")
        self._sim.reset(mask=mask, positions=positions)
        if self._spawner is not None and positions is None:      # the reset slots start by the spawner's rule; fallbacks keep the spawn above
            self._spawner.place_reset(mask)
        if self._tracker is not None:
            self._tracker.abandon(mask)
        return self._obs(), {a: {} for a in self.possible_agents}

    def step(self, actions, repeat: Optional[int] = None):
        """``actions``: int tensor ``[num_envs, A]`` or ``{agent_id: tensor[num_envs]}``.  ``repeat``: env ticks per call with the
        actions held (default: the constructor's ``frame_skip``); above 1, ``infos["ticks"]`` holds the ticks each slot played."""
        repeat = self._repeat(repeat)
        if isinstance(actions, dict):
            for i, aid in enumerate(self.possible_agents):
                self._actions[:, i] = actions[aid].reshape(self.num_envs).to(self._actions.dtype)
            acts = self._actions
        else:
            acts = actions
        # one launch: finished episodes are reset inside the tick kernel, which leaves the NEW episode's first
        # observations in the buffers of those slots (rewards / flags / winner are the terminal tick's)
        out = self._step_sim(acts, repeat)
        rewards = {aid: out["reward"][:, i] for i, aid in enumerate(self.possible_agents)}
        terminated, truncated = out["terminated"].bool(), out["truncated"].bool()   # fresh tensors
        infos = {"winner": out["winner"].clone(), "terminated": terminated, "truncated": truncated}
        if repeat > 1:
            infos["ticks"] = out["ticks"].clone()
        if self._final_pos is not None:
            infos["final_positions"] = self._final_pos      # a view: rows without ``terminated`` are not written (see the class docstring)
        terminations = {aid: terminated for aid in self.possible_agents}
        truncations = {aid: truncated for aid in self.possible_agents}
        return self._obs(), rewards, terminations, truncations, infos

    def state(self) -> Dict[str, Dict[str, torch.Tensor]]:
        o = self._sim.out
        nc = len(self.cops)
        res = {}
        for i, aid in enumerate(self.possible_agents):
            team = 0 if i < nc else 1
            sl = slice(0, nc) if team == 0 else slice(nc, None)
            res[aid] = {"own_obj_types": o["obs_type"][:, i], "own_distances": o["obs_distance"][:, i],
                        "object_type_shared": o["shared_type"][:, team], "distance_shared": o["shared_distance"][:, team],
                        "team_positions": o["team_positions"][:, sl]}
        return res

    def observations(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """The per-agent observation dictionaries over the current output buffers (what ``step`` / ``reset`` return)."""
        return self._obs()

    def step_raw(self, actions: torch.Tensor, repeat: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``step`` without the per-agent dictionaries: one launch (tick + auto-reset), returns the output buffers
        themselves (``raw_outputs()``): reward fp32 [N, A], terminated / truncated u8 [N], winner, observations.
        ``repeat`` as in ``step``; above 1 the buffers also carry ``ticks`` int32 [N]."""
        return self._step_sim(actions, self._repeat(repeat))

    def raw_outputs(self) -> Dict[str, torch.Tensor]:
        """The env core's output buffers as they lie on the device (``include/cat_sim.h`` ``cat_outputs``: f16 distances,
        u8 types, [N, A, R] / [N, 2, R]): what ``_obs()`` / ``state()`` slice per agent, for callers that pack the model
        inputs themselves (``include/cat_rollout.h``)."""
        return self._sim.out

    def random_actions(self, tick: int) -> torch.Tensor:
        return self._sim.random_actions(tick, out=self._actions)

    def rollout_random(self, ticks: int, tick0: int = 0) -> Dict[str, torch.Tensor]:
        """``ticks`` env ticks under uniformly random actions -- what ``driver.py:65-69`` does tick by tick with
        ``action_space(agent).sample()`` and skrl's trainer for ``random_timesteps`` (``mappo_config.py:9``) -- as ONE resident
        launch (``cat_rollout_fused``: the map stays in LDS, the state records stay in LDS) for the first ``ticks - 1`` ticks, whose
        outputs nobody reads (NULL output pointers: nothing is stored), and one ordinary step for the last, which leaves the
        ``[N, ...]`` output buffers as ``step`` does.  The actions are the synthetic Philox draws of ticks ``tick0 .. tick0 + ticks - 1``
        (``cat_random_actions``).  Returns the raw output buffers (``raw_outputs()``).

        With ``track_episodes`` the resident ticks keep their reward / terminated / truncated / winner rows (4 A + 3 bytes per env-tick;
        the observation pointers stay NULL) in ``[T, N, ...]`` buffers of at most ``TRACKED_ROLLOUT_BYTES`` (64 MiB: 1092 ticks of 4096
        envs of 3 agents per launch, never more than ``CAT_MAX_ROLLOUT_TICKS``), and the tracker takes each chunk in one launch."""
        ticks = int(ticks)
        if ticks < 1:
            raise ValueError("ticks must be >= 1")
        if self._spawner is not None:
            raise ValueError("rollout_random with a spawner attached: the resident launch cannot respawn between its ticks (step tick by tick, or set_spawner(None))")
        done, cap = 0, 65536
        keys = self._tracked_keys()
        if keys:
            cap = max(1, min(cap, self.TRACKED_ROLLOUT_BYTES // (self.num_envs * self._tracked_row_bytes(keys))))
        while ticks - 1 - done > 0:
            n = min(cap, ticks - 1 - done)
            rows = {} if not keys else self._tracked_rollout_rows(min(cap, ticks - 1), n, keys)
            if self._final_pos is not None:     # the resident launch's [T, N, A, 2] twin where a tracker reads it, else nothing (nobody sees these rows)
                twin = self._final_rollout_rows(min(cap, ticks - 1), n) if self._positions is not None else None
                self._sim.bind_final_positions(twin)
            try:
                self._sim.rollout_fused(n, None, tick=tick0 + done, auto_reset=self.auto_reset, out=rows)
            finally:
                if self._final_pos is not None:
                    self._sim.bind_final_positions(self._final_pos)
            if self._final_pos is not None and self._positions is not None:
                rows = dict(rows, final_positions=twin)
            self._track(rows)
            done += n
        out = self._sim.step_fused(None, tick=tick0 + ticks - 1, auto_reset=self.auto_reset)
        self._track(out)
        self._sim.check_errors()   # thousands of ticks went by inside one launch: a flag raised by any of them ends the run here, not never
        return out

    def _tracked_keys(self) -> tuple:
        """The output rows a tracked ``rollout_random`` keeps: the episode tracker's reward / flags, and with ``track_positions`` the
        terminated flags, ``team_positions`` and (with exposure) ``obs_type``."""
        keys = ("reward", "terminated", "truncated", "winner") if self._tracker is not None else ()
        if self._positions is not None:
            keys += tuple(k for k in ("terminated", "team_positions") if k not in keys) + (("obs_type",) if self._exposure else ())
            if self._final_pos is not None and "truncated" not in keys:
                keys += ("truncated",)
        return keys

    def _tracked_row_bytes(self, keys) -> int:
        """Bytes one env-tick of the kept rows takes (4 A + 3 for the episode tracker's alone)."""
        from .sim import _OUT_SPEC
        A, R = len(self.possible_agents), self._cfg.n_rays
        final = 4 * A if self._final_pos is not None and self._positions is not None else 0     # the [T, N, A, 2] f16 twin
        return final + sum(int(np.prod(_OUT_SPEC[k][0](1, A, R))) * torch.empty((), dtype=_OUT_SPEC[k][1]).element_size() for k in keys)

    def _tracked_rollout_rows(self, rows: int, n: int, keys=("reward", "terminated", "truncated", "winner")) -> Dict[str, torch.Tensor]:
        """The first ``n`` rows of the ``[rows, N, ...]`` buffers of a tracked ``rollout_random`` (kept, and grown when a longer chunk
        comes)."""
        from .sim import _OUT_SPEC
        if not self._tracked_rows or self._tracked_rows[keys[0]].shape[0] < rows:
            N, A, R = self.num_envs, len(self.possible_agents), self._cfg.n_rays
            self._tracked_rows = {k: torch.zeros((rows,) + tuple(_OUT_SPEC[k][0](N, A, R)), dtype=_OUT_SPEC[k][1], device=self.device)
                                  for k in keys}
        return {k: self._tracked_rows[k][:n] for k in keys}

    def _final_rollout_rows(self, rows: int, n: int) -> torch.Tensor:
        """The first ``n`` rows of the ``[rows, N, A, 2]`` end-of-episode buffer of a tracked ``rollout_random`` (kept, grown when a longer
        chunk comes, NaN-filled when made: the tracker reads terminal rows only, and those the launch writes)."""
        from .sim import FINAL_POS_NAN
        if self._final_rows is None or self._final_rows.shape[0] < rows:
            self._final_rows = torch.full((rows, self.num_envs, len(self.possible_agents), 2), FINAL_POS_NAN, dtype=torch.int16,
                                          device=self.device).view(torch.float16)
        return self._final_rows[:n]

    def render(self, env_ids: Optional[Sequence[int]] = None, rays: bool = False) -> torch.Tensor:
        """``rgb_array`` frames of the env slots ``env_ids`` (default ``[0]``), drawn on the GPU in one launch
        (``render_gpu.RenderScene``): a ``torch.uint8 [len(env_ids), W, H, 3]`` tensor on the env's device, x-major like
        ``BaseEnv.render``, W x H the largest map window of the batch (a slot's frame is white beyond its own map's window).
        ``rays=True`` also draws every agent's ray fan from the current observation buffers, coloured by what each ray hit.
        Read-only: the positions come from ``cat_get_state`` (position field only), the rays from the output buffers."""
        ids = [0] if env_ids is None else [int(e) for e in env_ids]
        if not ids:
            raise ValueError("render: env_ids is empty")
        bad = [e for e in ids if not 0 <= e < self.num_envs]
        if bad:
            raise IndexError(f"render: env ids {bad} outside [0, {self.num_envs})")
        if self._render_scene is None:
            from .render_gpu import RenderScene
            self._render_scene = RenderScene(self._compiled, self.device, sensor=self._cfg.sensor, agent_radius=self._cfg.agent_radius)
        sel = torch.tensor(ids, dtype=torch.long, device=self.device)
        pos = self._sim.get_positions().index_select(0, sel)
        ray_data = None
        if rays:
            o = self._sim.out
            ray_data = (o["obs_distance"].index_select(0, sel), o["obs_type"].index_select(0, sel))
        return self._render_scene.frames(self.slot_map_ids[ids], pos, rays=ray_data)

    def check_errors(self) -> None:
        """The step launches are asynchronous and cannot raise; this synchronises and raises ``ValueError`` if any
        action since the last check was outside ``Discrete(4)`` (the reference raises at once), ``CatSimError`` if a
        wall contact had to be dropped."""
        self._sim.check_errors()

    def get_env_state(self, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Full simulator state (bodies, caches, counters) for checkpointing: a copy on the device, no synchronisation.  ``out``: the
        dictionary an earlier call returned, overwritten instead of allocating a new one."""
        return self._sim.get_state(out)

    def set_env_state(self, **arrays) -> None:
        self._sim.set_state(**arrays)

    def close(self) -> None:
        self._sim.close()
