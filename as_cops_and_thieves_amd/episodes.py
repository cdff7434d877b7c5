"""Episode accounting: returns, lengths and outcomes of the episodes an env batch plays, added up where the data lies.

The env core writes, every tick, a reward per agent and ``terminated`` / ``truncated`` / ``winner`` per slot.  ``EpisodeTracker``
owns the per-slot state of ``include/cat_episodes.h`` for ``(num_envs, agents, max_step_count, device)`` and adds those streams up
into episodes.  On a GPU device ``update`` and ``summary`` are one kernel launch each on the current stream (no host
synchronisation in ``update``: it can be captured in a HIP graph with the env tick it follows; ``summary`` makes one, the copy of
its result).  On CPU tensors the same arithmetic runs in NumPy in the same order -- f64 adds in tick order inside a slot, the fixed
halving tree across the slots -- so the two agree bit for bit: the CPU trainer tests run on it, and the GPU tests hold the kernels
against it.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _learn_native as ln

HIST_BINS = ln.EPISODES_HIST_BINS
INT32_MAX = 2 ** 31 - 1
_BLOCK_BYTES = C.sizeof(ln.EpisodesSummaryBlock)
_INT_TOTALS = ("finished", "cop_wins", "thief_wins", "timeouts", "len_sum", "len_max")


def halving_tree_sum(x: np.ndarray) -> np.ndarray:
    """Sum of ``x`` [N, ...] over its first axis in the order ``cat_episodes_summary`` uses: pad with zeros to the next power of two
    P, then ``x[i] += x[i + h]`` for h = P/2, P/4, ..., 1."""
    n = x.shape[0]
    P = 1
    while P < n:
        P *= 2
    buf = np.zeros((P,) + x.shape[1:], dtype=x.dtype)
    buf[:n] = x
    h = P // 2
    while h >= 1:
        buf[:h] += buf[h:2 * h]
        h //= 2
    return buf[0].copy()


class EpisodeTracker:
    """Per-slot episode state and its totals (``include/cat_episodes.h``).  ``agents``: the env's agent ids (cops first), which name
    the ``mean_return/<agent>`` entries of ``summary()``."""

    def __init__(self, num_envs: int, agents: Sequence[str], max_step_count: int, device=None):
        self.N, self.agents, self.A = int(num_envs), list(agents), len(agents)
        self.max_step_count = int(max_step_count)
        self.device = torch.device("cpu" if device is None else device)
        if self.N < 1 or not 1 <= self.A <= ln.EPISODES_MAX_AGENTS or self.max_step_count < 1:
            raise ValueError(f"EpisodeTracker: num_envs >= 1, 1..{ln.EPISODES_MAX_AGENTS} agents and max_step_count >= 1 are required")
        N, A, dev = self.N, self.A, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        # the summary block and the histogram share one allocation: summary() brings both to the host in one copy
        self._tail = z((_BLOCK_BYTES + 8 * HIST_BINS,), torch.uint8)
        self.state: Dict[str, torch.Tensor] = {
            "ret_run": z((N, A), torch.float64), "len_run": z((N,), torch.int32), "finished": z((N,), torch.int32),
            "cop_wins": z((N,), torch.int32), "thief_wins": z((N,), torch.int32), "timeouts": z((N,), torch.int32),
            "len_sum": z((N,), torch.int64), "len_min": torch.full((N,), INT32_MAX, dtype=torch.int32, device=dev),
            "len_max": z((N,), torch.int32), "ret_sum": z((N, A), torch.float64), "ret_sq": z((N, A), torch.float64),
            "len_hist": self._tail[_BLOCK_BYTES:].view(torch.int64)}
        # ONE quota buffer for the tracker's life (INT32_MAX = no limit): the update launch takes its pointer by value, so a launch
        # captured in a HIP graph keeps reading this buffer, and set_quota after the capture reaches the replays
        self._quota = torch.full((N,), INT32_MAX, dtype=torch.int32, device=dev)
        self._limited = False
        self._gpu = dev.type == "cuda"
        self._seg_out = None                       # device blocks of segment_blocks(), made at its first call
        if self._gpu:
            ln.lib()     # a missing kernel library is an error here, not at the first update

    # ------------------------------------------------------------------ feeding
    def update(self, reward, terminated, truncated, winner, ticks=None) -> None:
        """One tick ``[N, ...]`` or T consecutive ticks ``[T, N, ...]`` of the env's outputs: reward ``[.., N, A]`` fp32,
        terminated / truncated ``[.., N]`` (uint8 or bool), winner ``[.., N]`` int8.

        ``ticks`` (int ``[.., N]``, every entry >= 1): the rows are frame-skip windows (``CatSim.step_repeat``) -- row t of slot n
        stands for ``ticks[t, n]`` env ticks, its reward is the window's fp32 sum and its flags are those of the window's last tick.
        The slot's length then grows by ``ticks`` instead of by 1, so lengths, the histogram, outcomes and counts equal those of
        tick-by-tick tracking.  A return is the f64 sum of the fp32 window sums in window order: it differs from the tick-by-tick f64
        sum in the last bits (the fp32 adds inside a window have already rounded)."""
        if reward.dim() == 2:
            reward, terminated, truncated, winner = reward[None], terminated[None], truncated[None], winner[None]
            ticks = None if ticks is None else ticks[None]
        T = reward.shape[0]
        if tuple(reward.shape) != (T, self.N, self.A) or any(tuple(t.shape) != (T, self.N) for t in (terminated, truncated, winner)):
            raise ValueError(f"EpisodeTracker.update: expected [T, {self.N}, {self.A}] rewards and [T, {self.N}] flags, got "
                             f"{tuple(reward.shape)}, {tuple(terminated.shape)}, {tuple(truncated.shape)}, {tuple(winner.shape)}")
        if ticks is not None and tuple(ticks.shape) != (T, self.N):
            raise ValueError(f"EpisodeTracker.update: expected [T, {self.N}] ticks, got {tuple(ticks.shape)}")
        if any(t.device != self.device for t in (reward, terminated, truncated, winner) + (() if ticks is None else (ticks,))):
            raise ValueError(f"EpisodeTracker.update: the streams must lie on {self.device}")
        as_u8 = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).contiguous()
        reward = reward.to(torch.float32).contiguous()
        terminated, truncated, winner = as_u8(terminated), as_u8(truncated), winner.to(torch.int8).contiguous()
        ticks = None if ticks is None else ticks.to(torch.int32).contiguous()
        if self._gpu:
            for t0 in range(0, T, ln.EPISODES_MAX_TICKS):
                sl = slice(t0, min(T, t0 + ln.EPISODES_MAX_TICKS))
                ln.episodes_update(self.state, reward[sl], terminated[sl], truncated[sl], winner[sl], self._quota, self.max_step_count,
                                   ticks=None if ticks is None else ticks[sl])
        else:
            self._update_host(reward.numpy(), terminated.numpy(), truncated.numpy(), winner.numpy(), None if ticks is None else ticks.numpy())

    def _update_host(self, reward, terminated, truncated, winner, ticks=None) -> None:
        """The kernel's arithmetic in NumPy, slots in parallel, ticks in order."""
        s = {k: v.numpy() for k, v in self.state.items()}       # views: updated in place
        quota = self._quota.numpy()
        for t in range(reward.shape[0]):
            s["ret_run"] += reward[t].astype(np.float64)
            s["len_run"] += 1 if ticks is None else ticks[t]
            term = terminated[t] != 0
            if not term.any():
                continue
            counted = term & (s["finished"] < quota)
            c = np.nonzero(counted)[0]
            if c.size:
                length = s["len_run"][c]
                s["finished"][c] += 1
                s["cop_wins"][c] += winner[t][c] == 0
                s["thief_wins"][c] += winner[t][c] == 1
                s["timeouts"][c] += truncated[t][c] != 0
                s["len_sum"][c] += length
                s["len_min"][c] = np.minimum(s["len_min"][c], length)
                s["len_max"][c] = np.maximum(s["len_max"][c], length)
                run = s["ret_run"][c]
                s["ret_sum"][c] += run
                s["ret_sq"][c] += run * run
                bins = np.minimum(HIST_BINS - 1, (length.astype(np.int64) - 1) * HIST_BINS // self.max_step_count)
                np.add.at(s["len_hist"], bins, 1)
            s["ret_run"][term] = 0.0
            s["len_run"][term] = 0

    def set_quota(self, quota) -> None:
        """How many episodes of each slot are counted: an int (every slot), an int tensor / sequence ``[N]``, or None (all).  Copied
        into the tracker's own buffer, so it also reaches update launches that were captured in a graph before."""
        self._limited = quota is not None
        if quota is None or isinstance(quota, int):
            self._quota.fill_(INT32_MAX if quota is None else quota)
        else:
            self._quota.copy_(torch.as_tensor(quota).to(torch.int32).reshape(self.N))

    @property
    def quota(self) -> Optional[torch.Tensor]:
        """The per-slot quota ``[N]`` int32, or None without one."""
        return self._quota if self._limited else None

    def abandon(self, mask=None) -> None:
        """Forget the episodes under way in the masked slots (all without a mask): one cut short by an explicit reset is not counted."""
        if mask is None:
            self.state["ret_run"].zero_()
            self.state["len_run"].zero_()
            return
        m = torch.as_tensor(mask).to(self.device).reshape(self.N) != 0
        self.state["ret_run"].masked_fill_(m.view(self.N, 1), 0.0)
        self.state["len_run"].masked_fill_(m, 0)

    def clear(self) -> None:
        """Zero the totals and the histogram; the episodes under way and the quota stay."""
        for k in _INT_TOTALS + ("ret_sum", "ret_sq", "len_hist"):
            self.state[k].zero_()
        self.state["len_min"].fill_(INT32_MAX)

    # ------------------------------------------------------------------ reading
    def summary_block(self) -> Dict[str, object]:
        """The raw totals (``cat_episodes_summary_block`` and the histogram) as Python numbers / lists: one synchronisation."""
        A = self.A
        if self._gpu:
            ln.episodes_summary(self.state, self.quota, self._tail)
            host = self._tail.cpu().numpy()
            blk = ln.EpisodesSummaryBlock.from_buffer_copy(host[:_BLOCK_BYTES].tobytes())
            out = {k: int(getattr(blk, k)) for k in ("episodes", "cop_wins", "thief_wins", "timeouts", "open_slots", "len_sum", "len_min", "len_max")}
            out["ret_sum"], out["ret_sq"] = [float(v) for v in blk.ret_sum[:A]], [float(v) for v in blk.ret_sq[:A]]
            out["len_hist"] = [int(v) for v in host[_BLOCK_BYTES:].view(np.int64)]
            return out
        s = {k: v.numpy() for k, v in self.state.items()}
        out = {"episodes": int(s["finished"].sum(dtype=np.int64)), "cop_wins": int(s["cop_wins"].sum(dtype=np.int64)),
               "thief_wins": int(s["thief_wins"].sum(dtype=np.int64)), "timeouts": int(s["timeouts"].sum(dtype=np.int64)),
               "open_slots": 0 if self.quota is None else int((s["finished"] < self.quota.numpy()).sum()),
               "len_sum": int(s["len_sum"].sum()), "len_min": int(s["len_min"].min()), "len_max": int(s["len_max"].max())}
        out["ret_sum"] = [float(v) for v in halving_tree_sum(s["ret_sum"])]
        out["ret_sq"] = [float(v) for v in halving_tree_sum(s["ret_sq"])]
        out["len_hist"] = [int(v) for v in s["len_hist"]]
        return out

    def summary(self) -> Dict[str, object]:
        """Totals of the counted episodes as Python numbers (one synchronisation).  With nothing counted yet the rates, means and
        the two length extremes are 0."""
        return self._derived(self.summary_block())

    def segment_blocks(self, bounds) -> List[Dict[str, object]]:
        """``summary_block()`` without the histogram for each of the contiguous slot segments ``bounds`` (S + 1 row bounds: 0 first, N
        last, strictly increasing, at most ``_learn_native.EPISODES_MAX_SEGMENTS`` segments; ValueError otherwise, before anything is
        launched).  On a GPU ONE launch (``cat_episodes_segment_summary``) and one copy; on CPU tensors ``halving_tree_sum`` per slice.
        A segment's block is bit for bit the ``summary_block()`` of a tracker that holds that segment's slots alone."""
        start = ln.segment_bounds(self.N, bounds)
        S, A = len(start) - 1, self.A
        ints = ("episodes", "cop_wins", "thief_wins", "timeouts", "open_slots", "len_sum", "len_min", "len_max")
        if self._gpu:
            if self._seg_out is None:
                self._seg_out = torch.zeros(ln.EPISODES_MAX_SEGMENTS * _BLOCK_BYTES, dtype=torch.uint8, device=self.device)
            ln.episodes_segment_summary(self.state, self.quota, start, self._seg_out)
            host = self._seg_out[:S * _BLOCK_BYTES].cpu().numpy().tobytes()
            out = []
            for k in range(S):
                blk = ln.EpisodesSummaryBlock.from_buffer_copy(host[k * _BLOCK_BYTES:(k + 1) * _BLOCK_BYTES])
                b = {f: int(getattr(blk, f)) for f in ints}
                b["ret_sum"], b["ret_sq"] = [float(v) for v in blk.ret_sum[:A]], [float(v) for v in blk.ret_sq[:A]]
                out.append(b)
            return out
        s = {k: v.numpy() for k, v in self.state.items()}
        quota = None if self.quota is None else self.quota.numpy()
        out = []
        for lo, hi in zip(start[:-1], start[1:]):
            sl = slice(lo, hi)
            b = {"episodes": int(s["finished"][sl].sum(dtype=np.int64)), "cop_wins": int(s["cop_wins"][sl].sum(dtype=np.int64)),
                 "thief_wins": int(s["thief_wins"][sl].sum(dtype=np.int64)), "timeouts": int(s["timeouts"][sl].sum(dtype=np.int64)),
                 "open_slots": 0 if quota is None else int((s["finished"][sl] < quota[sl]).sum()),
                 "len_sum": int(s["len_sum"][sl].sum()), "len_min": int(s["len_min"][sl].min()), "len_max": int(s["len_max"][sl].max())}
            b["ret_sum"] = [float(v) for v in halving_tree_sum(s["ret_sum"][sl])]
            b["ret_sq"] = [float(v) for v in halving_tree_sum(s["ret_sq"][sl])]
            out.append(b)
        return out

    def segment_summary(self, bounds) -> List[Dict[str, object]]:
        """``summary()`` per contiguous slot segment (``bounds``: see ``segment_blocks``): a list of dicts with ``summary()``'s keys minus
        ``length_hist`` (the histogram stays global).  One synchronisation."""
        return [self._derived(b) for b in self.segment_blocks(bounds)]

    def _derived(self, b: Dict[str, object]) -> Dict[str, object]:
        """Rates, means and deviations of a raw block (``length_hist`` where the block carries the histogram)."""
        n = b["episodes"]
        out = {"episodes": n, "cop_wins": b["cop_wins"], "thief_wins": b["thief_wins"], "timeouts": b["timeouts"],
               "cop_win_rate": b["cop_wins"] / n if n else 0.0, "mean_length": b["len_sum"] / n if n else 0.0,
               "min_length": b["len_min"] if n else 0, "max_length": b["len_max"]}
        for i, a in enumerate(self.agents):
            mean = b["ret_sum"][i] / n if n else 0.0
            out[f"mean_return/{a}"] = mean
            out[f"std_return/{a}"] = math.sqrt(max(0.0, b["ret_sq"][i] / n - mean * mean)) if n else 0.0
        if "len_hist" in b:
            out["length_hist"] = b["len_hist"]
        out["open_slots"] = b["open_slots"]
        return out

    def per_slot(self) -> Dict[str, torch.Tensor]:
        """The raw per-slot tensors (``cat_episodes_state``) and the quota, as they lie on the device."""
        return dict(self.state, quota=self.quota)
