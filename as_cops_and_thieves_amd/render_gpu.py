"""Batched ``rgb_array`` frames on the GPU (``include/cat_render.h``, in ``libcat_learn.so``).

``RenderScene`` uploads the geometry of a list of ``CompiledMap`` once; ``frames`` then draws F frames in one launch straight from
device buffers (positions, and optionally the env core's observation buffers for the ray fans).  Every frame is byte-equal to
``render.render_frame_reference`` (``render.render_rgb_array`` without rays) over its map's window, and 255 beyond it: the frames of
one call share the size of the scene's largest window.  There is no CPU path: without a GPU or the built library this raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _learn_native as ln
from . import tables
from .constants import DEFAULT_PHYSICAL, DEFAULT_SENSOR, SensorParams
from .maps import CompiledMap


class RenderScene:
    """The maps of a batch on one device, for ``frames``.  ``sensor`` gives the ray table (``tables.ray_table``) and the ray length
    the observation distances are measured against; all maps must share one roster (``n_cops`` of the colour split)."""

    def __init__(self, compiled_maps: Sequence[CompiledMap], device=None, *, sensor: SensorParams = DEFAULT_SENSOR,
                 agent_radius: float = DEFAULT_PHYSICAL.unit_size):
        maps = list(compiled_maps)
        if not maps:
            raise ValueError("RenderScene needs at least one map")
        if any((m.n_cops, m.n_thieves) != (maps[0].n_cops, maps[0].n_thieves) for m in maps):
            raise ValueError("all maps of a scene must share one roster")
        if not torch.cuda.is_available():
            raise RuntimeError("RenderScene draws on the GPU and no HIP device is visible to torch")
        self._L = ln.lib()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device must be a GPU, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device, self.maps = dev, maps
        self.n_cops, self.n_agents = maps[0].n_cops, maps[0].n_agents
        self.agent_radius = float(agent_radius)
        self.ray_length = float(sensor.ray_length)
        self.ray_dx, self.ray_dy = tables.ray_table(sensor)
        self.n_rays = int(sensor.num_rays)
        win = np.array([[int(m.window[0]), int(m.window[1])] for m in maps], dtype=np.int32)
        off = np.zeros(len(maps) + 1, dtype=np.int32)
        off[1:] = np.cumsum([m.n_shapes for m in maps])
        plane_off = np.cumsum([0] + [m.n_planes for m in maps])[:-1]
        first = np.concatenate([m.shape_first.astype(np.int64) + po for m, po in zip(maps, plane_off)]).astype(np.int32)
        count = np.concatenate([m.shape_count for m in maps]).astype(np.int32)
        bb = np.concatenate([m.shape_bb.reshape(-1, 4) for m in maps]).astype(np.float64)
        planes = np.ascontiguousarray(np.concatenate([m.planes.reshape(-1, 8)[:, :5] for m in maps]), dtype=np.float64)
        self.width, self.height = int(win[:, 0].max()), int(win[:, 1].max())
        self._host = {"window": win, "shape_off": off}                   # kept alive: the library reads them at every call

        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev)
        self._dev = {"window": up(win), "shape_off": up(off), "shape_bb": up(bb), "shape_first": up(first),
                     "shape_count": up(count), "planes": up(planes), "ray_dx": up(self.ray_dx), "ray_dy": up(self.ray_dy)}
        d = self._dev
        self._scene = ln.RenderSceneDesc(len(maps), self.n_rays, d["window"].data_ptr(), win.ctypes.data, d["shape_off"].data_ptr(),
                                         off.ctypes.data, d["shape_bb"].data_ptr(), d["shape_first"].data_ptr(),
                                         d["shape_count"].data_ptr(), d["planes"].data_ptr(), d["ray_dx"].data_ptr(),
                                         d["ray_dy"].data_ptr())

    def rays_of(self, distance, obj_type):
        """The ``rays`` tuple of ``render.render_frame_reference`` for one frame's [A, R] observation rows (host arrays)."""
        return (self.ray_dx, self.ray_dy, self.ray_length, np.asarray(distance), np.asarray(obj_type))

    def frames(self, map_ids, positions, rays=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Draw F frames: ``map_ids`` [F] (indices into the scene's maps), ``positions`` f64 [F, A, 2] (cops first), ``rays`` None or
        ``(obs_distance f16 [F, A, R], obs_type u8 [F, A, R])`` on the device.  Returns (or fills ``out``, a C-contiguous
        ``torch.uint8 [F, W, H, 3]`` on the device) the frames, W x H the scene's largest window.  Asynchronous on the current stream."""
        ids = np.ascontiguousarray(torch.as_tensor(map_ids).cpu().numpy().reshape(-1), dtype=np.int32)
        F, A = int(ids.shape[0]), self.n_agents
        if F == 0:
            raise ValueError("frames: no frames asked for")
        pos = torch.as_tensor(positions).to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(pos.shape) != (F, A, 2):
            raise ValueError(f"positions must have shape {(F, A, 2)}, got {tuple(pos.shape)}")
        shape = (F, self.width, self.height, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous torch.uint8 tensor of shape {shape} on {self.device}")
        flags, dist, typ = 0, None, None
        if rays is not None:
            dist, typ = rays
            want = (F, A, self.n_rays)
            dist = torch.as_tensor(dist).to(device=self.device).contiguous()
            typ = torch.as_tensor(typ).to(device=self.device, dtype=torch.uint8).contiguous()
            if tuple(dist.shape) != want or tuple(typ.shape) != want or dist.dtype != torch.float16:
                raise ValueError(f"rays must be (float16 {want}, uint8 {want})")
            flags = ln.RENDER_RAYS
        ids_dev = torch.from_numpy(ids).to(self.device, non_blocking=False)
        a = ln.RenderArgs(F, self.width, self.height, flags, self.n_cops, A, self.n_rays, 0, self.agent_radius, self.ray_length,
                          ids.ctypes.data, ids_dev.data_ptr(), pos.data_ptr(), 0 if dist is None else dist.data_ptr(),
                          0 if typ is None else typ.data_ptr(), out.data_ptr())
        stream = torch.cuda.current_stream(self.device).cuda_stream   # (temporaries made here are freed in this stream's order)
        ln._check(self._L.cat_render_frames(C.byref(self._scene), C.byref(a), C.c_void_p(stream)), "cat_render_frames")
        return out
