"""Shared by tests/test_positions_host.py and tests/test_gpu_positions.py (test infrastructure): a plain per-row Python statement of
the position-counting rule, and the synthetic streams both files feed."""
from __future__ import annotations

import math

import numpy as np

OCC, SEEN, SPAWN = 0, 1, 2
COP, THIEF = 1, 2


def loop_reference(pos, terminated, obs_type, group, quota, n_cops, cell, Wc, Hc, G, state=None):
    """The rule of include/cat_render.h, one row, one slot, one agent at a time, in Python numbers.  pos f16 [T, N, A, 2]; terminated
    [T, N]; obs_type u8 [T, N, A, R] or None; group / quota int [N] or None.  ``state``: the dict an earlier call returned, continued."""
    T, N, A, _ = pos.shape
    if state is None:
        state = {"counts": np.zeros((G, 3, A, Wc, Hc), np.int64), "outside": np.zeros((G, A), np.int64), "rows": np.zeros(G, np.int64),
                 "done": np.zeros(N, np.int32)}
    counts, outside, rows, done = state["counts"], state["outside"], state["rows"], state["done"]
    for t in range(T):
        for n in range(N):
            g = 0 if group is None else int(group[n])
            if g < 0:
                continue
            if quota is not None and done[n] >= quota[n]:
                continue
            rows[g] += 1
            term = terminated[t, n] != 0
            for a in range(A):
                x, y = float(pos[t, n, a, 0]), float(pos[t, n, a, 1])
                valid = math.isfinite(x) and math.isfinite(y) and x >= 0 and y >= 0
                if valid:
                    cx, cy = int(math.floor(x)) // cell, int(math.floor(y)) // cell
                    valid = cx < Wc and cy < Hc
                if not valid:
                    outside[g, a] += 1
                elif term:
                    counts[g, SPAWN, a, cx, cy] += 1
                else:
                    counts[g, OCC, a, cx, cy] += 1
                    if obs_type is not None:
                        code = COP if a < n_cops else THIEF
                        others = range(n_cops, A) if a < n_cops else range(n_cops)
                        if any(int(k) == code for b in others for k in obs_type[t, n, b]):
                            counts[g, SEEN, a, cx, cy] += 1
            done[n] += int(term)
    return state


def synthetic_stream(seed, T, N, A, R, W, H, G):
    """Fixed-seed rows: positions as a random walk of at most 2 px per tick and axis, with a 5 % share of teleports and a 5 % share of
    NaN / inf / negative values; sparse obs_type bytes in 0..6; terminal rows with probability 0.15; random groups in -1 .. G-1; quotas
    (7 n) % 5."""
    rng = np.random.default_rng(seed)
    walk = rng.uniform(0, 1, size=(N, A, 2)) * np.array([W, H])
    pos = np.zeros((T, N, A, 2), np.float16)
    for t in range(T):
        walk = walk + rng.uniform(-2.0, 2.0, size=walk.shape)
        jump = rng.random((N, A)) < 0.05
        walk[jump] = rng.uniform(0, 1, size=(int(jump.sum()), 2)) * np.array([W, H])
        walk = np.clip(walk, 0.0, [W - 0.01, H - 0.01])
        row = walk.astype(np.float32).copy()
        bad = rng.random((N, A)) < 0.05
        kind = rng.integers(0, 5, size=(N, A))
        axis = rng.integers(0, 2, size=(N, A))
        for v, value in enumerate((np.nan, np.inf, -np.inf, -3.5, None)):
            m = bad & (kind == v)
            idx = np.nonzero(m)
            row[idx[0], idx[1], axis[m]] = (W + H + 7.0) if value is None else value      # (None: beyond the grid on either axis)
        pos[t] = row.astype(np.float16)
    terminated = (rng.random((T, N)) < 0.15).astype(np.uint8)
    obs_type = np.where(rng.random((T, N, A, R)) < 0.03, rng.integers(0, 7, size=(T, N, A, R)), 4).astype(np.uint8)
    group = rng.integers(-1, G, size=N).astype(np.int32)
    quota = ((7 * np.arange(N)) % 5).astype(np.int32)
    return pos, terminated, obs_type, group, quota
