#!/usr/bin/env python3
"""Frames per second of the batched GPU renderer (include/cat_render.h) against the NumPy reference.

For labyrinth and agh-map, F in {1, 16, 256} frames per launch, with and without the ray fans: F env slots are stepped 50 random
ticks, then ``VecCopsEnv.render`` draws them.  The kernel is timed with device events around ``--iters`` launches of
``RenderScene.frames`` after warm-up (inputs already on the device, so the window holds the launches alone); the write bandwidth is
F * W * H * 3 bytes over that time, compared with the HBM figures of the MI355X (8.0 TB/s spec, ~6.3 TB/s measured by a streaming
copy).  The NumPy figure is ``render_frame_reference`` on the host, per frame, for the same frames (a few of them: it is slow).

    python tools/render_bench.py [--iters 50] [--out profiles/render_bench.txt]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from as_cops_and_thieves_amd.environments import VecCopsEnv  # noqa: E402
from as_cops_and_thieves_amd.maps import load_preset  # noqa: E402
from as_cops_and_thieves_amd.render import render_frame_reference  # noqa: E402

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--numpy-frames", type=int, default=3)
    ap.add_argument("--maps", default="labyrinth,agh-map")
    ap.add_argument("--frames", default="1,16,256")
    ap.add_argument("--num-rays", type=int, default=90)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# render_bench: {torch.cuda.get_device_name(0)}, {args.iters} timed launches per row after warm-up, {args.num_rays} rays",
             f"{'map':10s} {'F':>4s} {'rays':>5s} {'us/launch':>10s} {'frames/s':>11s} {'GB/s':>8s} {'%HBM(6.29)':>10s} "
             f"{'numpy ms/frame':>15s} {'speed-up':>9s}"]
    print(lines[0], flush=True)
    print(lines[1], flush=True)
    for name in args.maps.split(","):
        preset = load_preset(name, 2, 1)
        for F in (int(v) for v in args.frames.split(",")):
            env = VecCopsEnv(preset, F, num_rays=args.num_rays, seed=1)
            env.reset()
            env.rollout_random(50)
            env.render(range(F), rays=True)                        # builds the scene
            scene = env._render_scene
            pos = env._sim.get_positions()
            out = env.raw_outputs()
            ids = env.slot_map_ids
            dist, typ = out["obs_distance"].clone(), out["obs_type"].clone()
            frames = torch.empty((F, scene.width, scene.height, 3), dtype=torch.uint8, device=env.device)
            host_pos = pos.cpu().numpy()
            for rays in (False, True):
                r = (dist, typ) if rays else None
                for _ in range(5):
                    scene.frames(ids, pos, rays=r, out=frames)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    scene.frames(ids, pos, rays=r, out=frames)
                t1.record()
                torch.cuda.synchronize()
                us = t0.elapsed_time(t1) * 1e3 / args.iters
                nbytes = F * scene.width * scene.height * 3
                bw = nbytes / (us * 1e-6)
                cm = env._compiled[0]
                hd, ht = dist.cpu().numpy(), typ.cpu().numpy()
                n_np = min(F, args.numpy_frames)
                s = time.perf_counter()
                wants = [render_frame_reference(cm, host_pos[k], cm.n_cops, scene.agent_radius,
                                                rays=scene.rays_of(hd[k], ht[k]) if rays else None) for k in range(n_np)]
                np_ms = (time.perf_counter() - s) * 1e3 / n_np
                got = frames[:n_np].cpu().numpy()
                same = all(np.array_equal(got[k, :w.shape[0], :w.shape[1]], w) for k, w in enumerate(wants))
                fps = F / (us * 1e-6)
                row = (f"{name:10s} {F:4d} {str(rays):>5s} {us:10.1f} {fps:11.0f} {bw / 1e9:8.1f} {100 * bw / HBM_MEASURED:9.1f}% "
                       f"{np_ms:15.2f} {np_ms * 1e3 * F / us:8.0f}x" + ("" if same else "  MISMATCH vs NumPy"))
                print(row, flush=True)
                lines.append(row)
            env.close()
    lines.append(f"# bound: F*W*H*3 bytes of writes at {HBM_MEASURED / 1e12:.2f} TB/s (1280x800: {1280 * 800 * 3 / HBM_MEASURED * 1e6:.2f} us "
                 f"per frame); spec {HBM_SPEC / 1e12:.1f} TB/s")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
