#!/usr/bin/env python3
"""What running value normalisation (TrainerConfig.value_norm) costs an update: profiles/value_norm.txt.

    python tools/value_norm_bench.py [--envs 4096] [--map labyrinth] [--horizon 128] [--reps 8] [--warmup 3] [--regs-only]
                                     [--parent-src FILE --parent-include DIR] [--out profiles/value_norm.txt]

Two trainers in one process, ``value_norm`` off (the code path of the parent commit, line for line: cat_ppo_gae_scan, no moments, no
extra buffer) and on (cat_ppo_gae_scan_scaled, the two launches of cat_ppo_moments, the normalisation of the targets), each over its
own env from the same seeds.  After ``--warmup`` collect + update rounds of each (eager rollout, capture, replay; the update's graphs),
every repetition measures both, the order alternating from repetition to repetition (off-on, on-off, ...):
  - update head, ms: device events from the start of ``update()`` (collection has ended) to the entry of the first minibatch step --
    bootstrap values, the scan, with the option the moments and the normalisation, the advantage normalisation, the relayout;
  - collect + update env-steps/s: host clock around ``collect(); update()`` that ends in a device synchronise.
Median and min .. max over the repetitions are recorded: the spread says what a difference is worth.  No threshold is set.
Section 2 needs no GPU: the tool compiles csrc/cat_ppo.hip for gfx950 with the library's flags (``_learn_native.HIPCC_FLAGS``) plus
``-Rpass-analysis=kernel-resource-usage`` and records the compiler's remarks for the scan's two instantiations and the moment kernels;
``--parent-src`` / ``--parent-include`` do the same for another copy of the file (the parent commit's, e.g. from ``git show``), so that the
plain scan can be held against what it was.  ``--regs-only`` writes section 2 alone and records section 1 as not taken."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def speed_section(a):
    import dataclasses
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
    rc = dataclasses.replace(CFG_AGENT, random_timesteps=0, learning_starts=0)
    out = [f"## 1. speed: {a.map} 2v1, {a.envs} envs, 64 rays, {a.horizon}-tick rollouts, bptt 16; {a.warmup} warm-up rounds, {a.reps} repetitions, order alternating",
           "#    median (min .. max)"]
    fmt = lambda v, p: f"{statistics.median(v):.{p}f} ({min(v):.{p}f} .. {max(v):.{p}f})"
    legs, first = {}, {}
    for on in (False, True):
        env = VecCopsEnv(load_preset(a.map, 2, 1), a.envs, num_rays=64, max_step_count=400, seed=1)
        tcfg = TrainerConfig(horizon=a.horizon, policy_freeze_duration=0, opponent_freeze_duration=0, value_norm=on)
        tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, tcfg, seed=0)
        legs[on] = (env, tr)
        first[on] = {"event": None}
        for rl in tr.roles.values():        # an event at the entry of the update's first minibatch step

            def step(use_graph, rl=rl, inner=rl.minibatch_step, slot=first[on]):
                if slot["event"] is None:
                    slot["event"] = torch.cuda.Event(enable_timing=True)
                    slot["event"].record()
                return inner(use_graph)
            rl.minibatch_step = step
    for _ in range(a.warmup):
        for on, (_, tr) in legs.items():
            tr.collect(); tr.update()
            first[on]["event"] = None
    torch.cuda.synchronize()
    res = {on: {"head_ms": [], "steps_s": []} for on in legs}
    for r in range(a.reps):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            _, tr = legs[on]
            assert tr._graph is not None, "the rollout is not captured"
            e0 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.collect()
            e0.record()
            tr.update()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[on]["head_ms"].append(e0.elapsed_time(first[on]["event"]))
            res[on]["steps_s"].append(a.horizon * a.envs / dt / 1e6)
            first[on]["event"] = None
    for on, label in ((False, "value_norm off"), (True, "value_norm on ")):
        out.append(f"{label}: update head {fmt(res[on]['head_ms'], 3)} ms   collect + update {fmt(res[on]['steps_s'], 3)} M env-steps/s")
    off, onv = (statistics.median(res[f]["head_ms"]) for f in (False, True))
    out.append(f"update head, on - off: {onv - off:+.3f} ms (medians); collect + update, on / off: "
               f"{statistics.median(res[True]['steps_s']) / statistics.median(res[False]['steps_s']):.4f}")
    stats = legs[True][1].read_stats()
    out.append("scale after these updates: " + "  ".join(f"{ag} mu {stats[f'value_mean/{ag}']:.4f} sigma {stats[f'value_std/{ag}']:.4f}" for ag in legs[True][1].agents))
    for env, _ in legs.values():
        env.check_errors()
        env.close()
    return out


def kernel_resources(src, include):
    """Lines "kernel: VGPRs, SGPRs, LDS, scratch, occupancy" of the gae / moment kernels of one copy of cat_ppo.hip, from the compiler's remarks."""
    from as_cops_and_thieves_amd import _learn_native as ln
    flags = [f for f in ln.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--cuda-device-only", "-S", f"-I{include}", f"-I{ln.PKG / 'csrc'}",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return [f"FAILED rc={r.returncode}: {' '.join(cmd)}"] + r.stderr.splitlines()[-5:]
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    out = []
    for k in rows:
        if "gae_kernel" in k["name"] or "moments_" in k["name"]:
            out.append(f"{k['name']:72s} VGPRs {k.get('VGPRs'):>3s}  SGPRs {k.get('TotalSGPRs'):>3s}  LDS {k.get('LDS'):>5s} B  scratch {k.get('ScratchSize')}  "
                       f"waves/SIMD {k.get('Occupancy')}")
    return out


def regs_section(a):
    from as_cops_and_thieves_amd import _learn_native as ln
    out = ["", "## 2. registers, LDS and scratch of csrc/cat_ppo.hip: the scan's two instantiations and the moment kernels",
           "#    (hipcc " + " ".join(f for f in ln.HIPCC_FLAGS if f not in ("-fPIC", "-shared")) + " -Rpass-analysis=kernel-resource-usage)", "this commit:"]
    out += kernel_resources(ln.PKG / "csrc" / "cat_ppo.hip", ln.ROOT / "include")
    if a.parent_src:
        out += ["parent commit (gae_kernel before it became a template):"] + kernel_resources(a.parent_src, a.parent_include or ln.ROOT / "include")
    else:
        out += ["parent commit: not taken (--parent-src FILE --parent-include DIR)"]
    return out


def main():
    import torch
    from bench import source_sha16
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--map", default="labyrinth")
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regs-only", action="store_true")
    ap.add_argument("--parent-src", default=None)
    ap.add_argument("--parent-include", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "value_norm.txt"))
    a = ap.parse_args()
    if not a.regs_only and not torch.cuda.is_available():
        sys.exit("value_norm_bench: no GPU; no speed is measured without one (--regs-only: the compiler's figures alone)")
    lines = [f"# running value normalisation (TrainerConfig.value_norm) against the learner without it; env-core source {source_sha16()}; "
             + ("no device" if a.regs_only else torch.cuda.get_device_name(0))]
    lines += (["## 1. speed", "not taken (--regs-only)"] if a.regs_only else speed_section(a)) + regs_section(a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
