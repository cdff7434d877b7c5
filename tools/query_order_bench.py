#!/usr/bin/env python3
"""Index order against tree order (bbtree_gate 1 / 2, DESIGN D2) on the BASELINE shapes: the tick kernel's own time (cat_arm_kernel_timing,
bench.py's timed_steps) one launch per tick, and per tick of the resident launch (T = 64, timed_rollout), same seeds, same Philox
actions.  With a diagnostic build of the library (tools/build_variant.sh NAME -DCAT_TREE_COUNTS, then CAT_SIM_LIB=build/var/NAME.so)
it also reports the share of rays whose walls' result took fan_chunk's slow path (the exact tree descent): cat_debug_tree_counts
counts the rays with a wall hit and those among them that descended.  Timings from a diagnostic build carry its atomics; take them
from the shipped library.
usage: tools/query_order_bench.py [--steps K] [--warmup W] [--only SUBSTRING]"""
import argparse
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = (   # BASELINE.json configs[1] (the headline), [2] (per-GPU shard), [3], [4], [0] batched -- as bench.py measures them
    ("labyrinth 2v1 x4096", dict(map="labyrinth", cops=2, thieves=1, envs=4096, rays=64)),
    ("agh-map 2v1 x4096", dict(map="agh-map", cops=2, thieves=1, envs=4096, rays=64)),
    ("grandbyrinth 3v2 x8192", dict(map="grandbyrinth", cops=3, thieves=2, envs=8192, rays=64)),
    ("five maps mixed 2v1 x16384", dict(map="mixed", cops=2, thieves=1, envs=16384, rays=64)),
    ("squarinth 1v1 x4096, 90 rays", dict(map="squarinth", cops=1, thieves=1, envs=4096, rays=90)),
)


def make_sim(shape, gate):
    import numpy as np
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.sim import CatSim
    if shape["map"] == "mixed":
        cmaps = [load_preset(n, shape["cops"], shape["thieves"]).compile() for n in ("agh-map", "grandbyrinth", "labyrinth", "lbirinth", "squarinth")]
        slot = (np.arange(shape["envs"]) % 5).astype(np.int32)
    else:
        cmaps, slot = [load_preset(shape["map"], shape["cops"], shape["thieves"]).compile()], None
    cfg = SimConfig(n_envs=shape["envs"], n_cops=shape["cops"], n_thieves=shape["thieves"], n_rays=shape["rays"], max_step_count=400, seed=0,
                    bbtree_gate=gate)
    return CatSim(cfg, cmaps, slot, device="cuda:0")


def main():
    import torch
    from bench import HipEvents, timed_rollout, timed_steps
    from as_cops_and_thieves_amd import _native
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    L = _native.lib()
    counts = hasattr(L, "cat_debug_tree_counts")
    hip = HipEvents()
    fence = torch.cuda.synchronize
    digest = hashlib.sha256(b"".join(f.read_bytes() for f in _native.sources())).hexdigest()[:16]   # the env core's sources (as bench.py hashes them)
    print(json.dumps({"source_sha16": digest, "library": str(_native.LIB_PATH.name),
                      "slow-path counters": counts, "steps": args.steps, "warmup": args.warmup}), flush=True)
    for name, shape in SHAPES:
        if args.only and args.only not in name:
            continue
        row = {"shape": name}
        for gate, key in ((1, "index"), (2, "tree")):
            sim = make_sim(shape, gate)
            sim.reset()
            if counts:
                z = (C.c_ulonglong * 2)()
                L.cat_debug_tree_counts(z, 1)
            _, one_tick, _, _ = timed_steps(sim, args.steps, args.warmup, fence, hip)
            _, resident, _ = timed_rollout(sim, 64, fence, hip, first_tick=args.steps + args.warmup + 1)
            row[key] = {"kernel": sim.one_tick_kernel, "one_tick_us": round(one_tick * 1e3, 2), "resident_us_per_tick": round(resident * 1e3, 2)}
            if counts and gate == 2:
                got = (C.c_ulonglong * 2)()
                L.cat_debug_tree_counts(got, 1)
                rays = (args.steps + args.warmup + 5 * 64) * shape["envs"] * (shape["cops"] + shape["thieves"]) * shape["rays"]
                row[key].update(rays_traced=rays, rays_with_a_wall_hit=int(got[0]), slow_path=int(got[1]),
                                slow_path_share_of_rays=round(got[1] / rays, 6), slow_path_share_of_hits=round(got[1] / max(got[0], 1), 6))
            sim.close()
        row["tree/index one-tick"] = round(row["tree"]["one_tick_us"] / row["index"]["one_tick_us"], 3)
        row["tree/index resident"] = round(row["tree"]["resident_us_per_tick"] / row["index"]["resident_us_per_tick"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
