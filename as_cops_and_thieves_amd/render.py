"""Headless ``rgb_array`` frame.

The reference's ``rgb_array`` mode returns ``pygame.surfarray.array3d`` of a surface it never
draws on (``base_env.py:505-507``): an all-zero ``(width, height, 3)`` uint8 array.  This
rasteriser keeps that shape/dtype convention but draws the scene (hull walls, cops blue, thieves
red — the colours of ``cop.py:30`` / ``thief.py:29``), which is what a user wants from a frame.

``render_frame_reference`` is the pixel contract of the batched GPU renderer (``include/cat_render.h``, ``render_gpu.RenderScene``):
the same frame, optionally with every agent's ray fan drawn between the walls and the discs.  ``write_png`` stores a frame with the
standard library alone.
"""
from __future__ import annotations

import struct
import zlib
from typing import Optional, Sequence

import numpy as np

from .maps import CompiledMap


def render_rgb_array(cmap: CompiledMap, positions: np.ndarray, n_cops: int, agent_radius: float) -> np.ndarray:
    W, H = int(cmap.window[0]), int(cmap.window[1])
    img = np.full((W, H, 3), 255, dtype=np.uint8)
    xs = np.arange(W, dtype=np.float64)[:, None] + 0.5
    ys = np.arange(H, dtype=np.float64)[None, :] + 0.5
    for s in range(cmap.n_shapes):
        f, c = int(cmap.shape_first[s]), int(cmap.shape_count[s])
        l, b, r, t = cmap.shape_bb[s]
        x0, x1 = max(int(l), 0), min(int(r) + 1, W)
        y0, y1 = max(int(b), 0), min(int(t) + 1, H)
        if x0 >= x1 or y0 >= y1:
            continue
        inside = np.ones((x1 - x0, y1 - y0), dtype=bool)
        for pl in cmap.planes[f:f + c]:
            inside &= (pl[0] * xs[x0:x1] + pl[1] * ys[:, y0:y1] - pl[4]) <= 1.0   # hull inflated by r = 1
        img[x0:x1, y0:y1][inside] = (60, 60, 60)
    for i, (px, py) in enumerate(np.asarray(positions, dtype=np.float64)):
        colour = (0, 0, 255) if i < n_cops else (255, 0, 0)
        x0, x1 = max(int(px - agent_radius) - 1, 0), min(int(px + agent_radius) + 2, W)
        y0, y1 = max(int(py - agent_radius) - 1, 0), min(int(py + agent_radius) + 2, H)
        if x0 >= x1 or y0 >= y1:
            continue
        disc = (xs[x0:x1] - px) ** 2 + (ys[:, y0:y1] - py) ** 2 <= agent_radius ** 2
        img[x0:x1, y0:y1][disc] = colour
    return img


# ray colour by ObjectType (WALL, COP, THIEF, MOVABLE, EMPTY); a type above EMPTY is drawn as EMPTY.  include/cat_render.h
# CAT_RENDER_RAY_COLOURS holds the same table for the kernel.
RAY_COLOURS = np.array([(255, 140, 0), (0, 170, 255), (255, 60, 160), (0, 160, 0), (190, 190, 190)], dtype=np.uint8)


def _segment_d2(X: np.ndarray, Y: np.ndarray, px: float, py: float, ex: float, ey: float) -> np.ndarray:
    """Squared distance from the pixel centres (X, Y) to the segment (px, py) - (ex, ey), in the contract's operation order."""
    vx, vy = ex - px, ey - py
    wx, wy = X - px, Y - py
    c1 = wx * vx + wy * vy
    c2 = vx * vx + vy * vy
    d_start = wx * wx + wy * wy
    ax, ay = X - ex, Y - ey
    d_end = ax * ax + ay * ay
    with np.errstate(divide="ignore", invalid="ignore"):
        u = c1 / c2
        qx, qy = wx - u * vx, wy - u * vy
        d_mid = qx * qx + qy * qy
    return np.where(c1 <= 0.0, d_start, np.where(c1 >= c2, d_end, d_mid))


def render_frame_reference(cmap: CompiledMap, positions: np.ndarray, n_cops: int, agent_radius: float,
                           rays: Optional[Sequence] = None) -> np.ndarray:
    """The frame the GPU renderer draws, as ``(W, H, 3)`` uint8 over the map's window.

    Without ``rays`` this is ``render_rgb_array``.  With ``rays = (ray_dx, ray_dy, ray_length, distance_f16[A, R], obj_type_u8[A, R])``
    the ray segments of every agent are drawn after the walls and before the discs, agent by agent and ray by ray (a later write wins):
    ray k of an agent at (px, py) runs to ``(px + t * ray_dx[k], py + t * ray_dy[k])`` with ``t = float64(distance) / ray_length``; a
    pixel of the window ``[int(min) - 1, int(max) + 2)`` of the segment's bounding box (clipped to the frame) is lit, in
    ``RAY_COLOURS[object_type]``, when its centre lies within 0.5 of the segment (squared distance ``<= 0.25``)."""
    if rays is None:
        return render_rgb_array(cmap, positions, n_cops, agent_radius)
    ray_dx, ray_dy, ray_length, distance, obj_type = rays
    ray_dx = np.asarray(ray_dx, dtype=np.float64)
    ray_dy = np.asarray(ray_dy, dtype=np.float64)
    distance = np.asarray(distance, dtype=np.float16)
    obj_type = np.asarray(obj_type, dtype=np.uint8)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
    A, R = distance.shape
    if pos.shape[0] != A or obj_type.shape != (A, R) or ray_dx.shape != (R,) or ray_dy.shape != (R,):
        raise ValueError(f"rays: distance / object_type must be [A={pos.shape[0]}, R] and the ray table [R]")
    img = render_rgb_array(cmap, pos[:0], n_cops, agent_radius)     # background and walls only
    W, H = img.shape[0], img.shape[1]
    ray_length = float(ray_length)
    for i in range(A):
        px, py = float(pos[i, 0]), float(pos[i, 1])
        for k in range(R):
            t = float(distance[i, k]) / ray_length
            ex, ey = px + t * float(ray_dx[k]), py + t * float(ray_dy[k])
            x0, x1 = max(int(min(px, ex)) - 1, 0), min(int(max(px, ex)) + 2, W)
            y0, y1 = max(int(min(py, ey)) - 1, 0), min(int(max(py, ey)) + 2, H)
            if x0 >= x1 or y0 >= y1:
                continue
            X = np.arange(x0, x1, dtype=np.float64)[:, None] + 0.5
            Y = np.arange(y0, y1, dtype=np.float64)[None, :] + 0.5
            lit = _segment_d2(X, Y, px, py, ex, ey) <= 0.25
            img[x0:x1, y0:y1][lit] = RAY_COLOURS[min(int(obj_type[i, k]), len(RAY_COLOURS) - 1)]
    xs = np.arange(W, dtype=np.float64)[:, None] + 0.5
    ys = np.arange(H, dtype=np.float64)[None, :] + 0.5
    for i, (px, py) in enumerate(pos):                                # the discs: render_rgb_array's rule and colours
        colour = (0, 0, 255) if i < n_cops else (255, 0, 0)
        x0, x1 = max(int(px - agent_radius) - 1, 0), min(int(px + agent_radius) + 2, W)
        y0, y1 = max(int(py - agent_radius) - 1, 0), min(int(py + agent_radius) + 2, H)
        if x0 >= x1 or y0 >= y1:
            continue
        disc = (xs[x0:x1] - px) ** 2 + (ys[:, y0:y1] - py) ** 2 <= agent_radius ** 2
        img[x0:x1, y0:y1][disc] = colour
    return img


def _heat_palette() -> np.ndarray:
    """256 colours from white (level 0) over yellow, orange and red to dark red (level 255): integer interpolation between anchors."""
    anchors = [(0, (255, 255, 255)), (64, (255, 237, 160)), (128, (254, 178, 76)), (192, (240, 59, 32)), (255, (128, 0, 38))]
    pal = np.zeros((256, 3), dtype=np.uint8)
    for (l0, c0), (l1, c1) in zip(anchors, anchors[1:]):
        for level in range(l0, l1 + 1):
            pal[level] = [c0[k] + (c1[k] - c0[k]) * (level - l0) // (l1 - l0) for k in range(3)]
    return pal


HEAT_PALETTE = _heat_palette()
HEATMAP_PLANES = ("occ", "seen", "hidden", "spawn")     # hidden = occ - seen
HEATMAP_END_PLANES = ("capture", "timeout")             # a tracker with final positions: where episodes ended


def render_heatmap(cmap: CompiledMap, plane: np.ndarray, cell: int, vmax: Optional[int] = None, palette: np.ndarray = HEAT_PALETTE) -> np.ndarray:
    """A count map of ``positions.PositionTracker`` (one ``[Wc, Hc]`` plane of one group and agent, x-major) over the map's window as a
    ``(W, H, 3)`` uint8 frame, on the host: pixel (x, y) is ``palette[min(255, plane[x // cell, y // cell] * 255 // vmax)]`` (level 0 when
    ``vmax == 0``; ``vmax`` None = the plane's maximum), and the walls of ``render_rgb_array`` are drawn on top in their grey."""
    W, H = int(cmap.window[0]), int(cmap.window[1])
    plane = np.asarray(plane)
    cell = int(cell)
    if plane.ndim != 2 or cell < 1 or plane.shape[0] * cell < W or plane.shape[1] * cell < H:
        raise ValueError(f"render_heatmap: a plane of {plane.shape} cells of {cell} px does not cover the {W}x{H} window")
    palette = np.asarray(palette, dtype=np.uint8)
    if palette.shape != (256, 3):
        raise ValueError("render_heatmap: the palette must be [256, 3] uint8")
    plane = plane.astype(np.int64)
    vmax = int(plane.max()) if vmax is None else int(vmax)
    level = np.minimum(255, plane * 255 // vmax) if vmax > 0 else np.zeros_like(plane)
    level = np.clip(level, 0, 255)
    img = palette[level[np.arange(W)[:, None] // cell, np.arange(H)[None, :] // cell]]
    walls = render_rgb_array(cmap, np.zeros((0, 2)), 0, 0.0)
    grey = (walls == 60).all(axis=2)
    img[grey] = (60, 60, 60)
    return img


def write_heatmaps(directory, tracker, maps, group_names: Optional[Sequence[str]] = None, group_maps: Optional[Sequence[int]] = None,
                   vmax: Optional[int] = None, palette: np.ndarray = HEAT_PALETTE, npz_name: str = "positions.npz") -> dict:
    """The maps of a ``positions.PositionTracker`` as pictures: ``{group}/{agent}_{occ|seen|hidden|spawn}.png`` (``write_png`` of
    ``render_heatmap``; hidden = occ - seen) under ``directory`` and the raw counts in ``positions.npz`` (``counts``, ``outside``, ``rows``,
    ``done``, ``cell``, ``agents``, ``groups``).  ``maps``: the batch's maps (``Map`` or ``CompiledMap``; one or a list); ``group_maps[g]``:
    the map group g is drawn over (default: the first); ``group_names``: the directory names (default ``group_0`` ..; None for a group
    that gets no pictures).  A tracker that keeps the capture / timeout maps (``final_positions=True``) also gets
    ``{group}/{agent}_{capture|timeout}.png`` and ``ends`` / ``ends_outside`` in the npz; any other tracker gets exactly the files and
    arrays above.  One synchronisation (``tracker.counts()``).  Returns those counts."""
    from pathlib import Path
    directory = Path(directory)
    maps = list(maps) if isinstance(maps, (list, tuple)) else [maps]
    compiled = [m if isinstance(m, CompiledMap) else m.compile() for m in maps]
    G = tracker.G
    names = [f"group_{g}" for g in range(G)] if group_names is None else [None if n is None else str(n) for n in group_names]
    which = [0] * G if group_maps is None else [int(m) for m in group_maps]
    if len(names) != G or len(which) != G or any(not 0 <= m < len(compiled) for m in which):
        raise ValueError(f"write_heatmaps: {G} groups need {G} names and {G} map indices below {len(compiled)}")
    c = tracker.counts()
    directory.mkdir(parents=True, exist_ok=True)
    extra = {k: c[k] for k in ("ends", "ends_outside") if k in c}
    np.savez_compressed(directory / npz_name, counts=c["counts"], outside=c["outside"], rows=c["rows"], done=c["done"], **extra,
                        cell=np.int64(tracker.cell), agents=np.array(tracker.agents), groups=np.array(["" if n is None else n for n in names]))
    for g in range(G):
        if names[g] is None:
            continue
        (directory / names[g]).mkdir(parents=True, exist_ok=True)
        for i, aid in enumerate(tracker.agents):
            occ, seen, spawn = c["counts"][g, 0, i], c["counts"][g, 1, i], c["counts"][g, 2, i]
            for plane_name, plane in zip(HEATMAP_PLANES, (occ, seen, occ - seen, spawn)):
                write_png(directory / names[g] / f"{aid}_{plane_name}.png", render_heatmap(compiled[which[g]], plane, tracker.cell, vmax, palette))
            if "ends" in c:
                for k, plane_name in enumerate(HEATMAP_END_PLANES):
                    write_png(directory / names[g] / f"{aid}_{plane_name}.png",
                              render_heatmap(compiled[which[g]], c["ends"][g, k, i], tracker.cell, vmax, palette))
    return c


def write_png(path, frame: np.ndarray) -> None:
    """Store a ``(W, H, 3)`` uint8 frame (x-major, as ``render_rgb_array`` returns it) as an 8-bit RGB PNG of W x H pixels, with
    ``zlib`` and ``struct`` only: one IDAT chunk, filter type 0 on every row."""
    frame = np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError(f"write_png wants a (W, H, 3) uint8 frame, got {frame.shape} {frame.dtype}")
    W, H = frame.shape[0], frame.shape[1]
    rows = np.ascontiguousarray(frame.transpose(1, 0, 2)).reshape(H, 3 * W)
    raw = np.concatenate([np.zeros((H, 1), dtype=np.uint8), rows], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
