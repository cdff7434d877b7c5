#!/usr/bin/env python3
"""What the learner's schedules on the device (RoleConfig.lr_schedule) cost an update: profiles/hyper_schedule.txt.

    python tools/hyper_schedule_bench.py [--envs 4096] [--map labyrinth] [--horizon 128] [--reps 8] [--warmup 3] [--regs-only]
                                         [--parent-src FILE --parent-include DIR] [--out profiles/hyper_schedule.txt]

Two trainers in one process, schedules off (the code path of the parent commit: cat_ppo_loss_grad / cat_ppo_adam_step with the numbers by
value, no block, no extra launch) and on (``lr_schedule="kl_adaptive"``: cat_ppo_loss_grad_dev / cat_ppo_adam_step_dev reading the hyper
block inside the two captured graphs, one cat_ppo_schedule_step launch per epoch), each over its own env from the same seeds.  After
``--warmup`` collect + update rounds of each (eager rollout, capture, replay; the update's graphs), every repetition measures both, the
order alternating from repetition to repetition (off-on, on-off, ...):
  - update, ms: device events around ``update()``;
  - collect + update env-steps/s: host clock around ``collect(); update()`` that ends in a device synchronise.
Median and min .. max over the repetitions are recorded.  No threshold is set in advance: the file states the off leg's own run-to-run
range and where the on leg's median falls.
Section 2 needs no GPU: the tool compiles csrc/cat_ppo.hip for gfx950 with the library's flags (``_learn_native.HIPCC_FLAGS``) plus
``-Rpass-analysis=kernel-resource-usage`` and records the compiler's remarks for the loss, gradient-norm and Adam kernels' instantiations and
the schedule kernel; ``--parent-src`` / ``--parent-include`` do the same for another copy of the file (the parent commit's, e.g. from
``git show``) and the tool says whether the by-value instantiations kept its VGPRs, SGPRs and scratch.  ``--regs-only`` writes section 2
alone and records section 1 as not taken."""
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
KERNELS = ("ppo_loss_kernel", "grad_norm_kernel", "adam_kernel", "schedule_kernel")


def speed_section(a):
    import dataclasses
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
    out = [f"## 1. speed: {a.map} 2v1, {a.envs} envs, 64 rays, {a.horizon}-tick rollouts, bptt 16; {a.warmup} warm-up rounds, {a.reps} repetitions, order alternating",
           "#    median (min .. max)"]
    fmt = lambda v, p: f"{statistics.median(v):.{p}f} ({min(v):.{p}f} .. {max(v):.{p}f})"
    legs = {}
    for on in (False, True):
        rc = dataclasses.replace(CFG_AGENT, random_timesteps=0, learning_starts=0, **({"lr_schedule": "kl_adaptive"} if on else {}))
        env = VecCopsEnv(load_preset(a.map, 2, 1), a.envs, num_rays=64, max_step_count=400, seed=1)
        tr = MAPPOTrainer(env, {"cop": rc, "thief": rc}, TrainerConfig(horizon=a.horizon, policy_freeze_duration=0, opponent_freeze_duration=0), seed=0)
        assert all(rl.scheduled == on and hasattr(rl, "hyper") == on for rl in tr.roles.values())
        legs[on] = (env, tr)
    for _ in range(a.warmup):
        for _, tr in legs.values():
            tr.collect(); tr.update()
    torch.cuda.synchronize()
    res = {on: {"update_ms": [], "steps_s": []} for on in legs}
    for r in range(a.reps):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            _, tr = legs[on]
            assert tr._graph is not None and all(rl._graphs for rl in tr.roles.values()), "the rollout or the step is not captured"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.collect()
            e0.record()
            tr.update()
            e1.record()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[on]["update_ms"].append(e0.elapsed_time(e1))
            res[on]["steps_s"].append(a.horizon * a.envs / dt / 1e6)
    for on, label in ((False, "schedules off        "), (True, "schedules on (kl_adaptive)")):
        out.append(f"{label}: update {fmt(res[on]['update_ms'], 3)} ms   collect + update {fmt(res[on]['steps_s'], 3)} M env-steps/s")
    for key, unit, p in (("update_ms", "ms", 3), ("steps_s", "M env-steps/s", 3)):
        off, onv = res[False][key], statistics.median(res[True][key])
        where = "inside" if min(off) <= onv <= max(off) else ("below" if onv < min(off) else "above")
        out.append(f"{key}: the off leg's own range is {min(off):.{p}f} .. {max(off):.{p}f} {unit} (median {statistics.median(off):.{p}f}); the on leg's median "
                   f"{onv:.{p}f} lies {where} it ({onv - statistics.median(off):+.{p}f} between the medians)")
    stats = legs[True][1].read_stats()
    out.append("learning rates after these updates: " + "  ".join(f"{ag} {stats[f'lr/{ag}']:.3g}" for ag in legs[True][1].agents))
    for env, _ in legs.values():
        env.check_errors()
        env.close()
    return out


def kernel_resources(src, include):
    """{kernel name: figures} of the loss / norm / Adam / schedule kernels of one copy of cat_ppo.hip, from the compiler's remarks."""
    from as_cops_and_thieves_amd import _learn_native as ln
    flags = [f for f in ln.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--cuda-device-only", "-S", f"-I{include}", f"-I{ln.PKG / 'csrc'}",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"FAILED rc={r.returncode}: {' '.join(cmd)}\n" + "\n".join(r.stderr.splitlines()[-5:]))
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = rows.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    return {n: k for n, k in rows.items() if any(want in n for want in KERNELS)}


def _row(name, k):
    return (f"{name:64s} VGPRs {k.get('VGPRs'):>3s}  SGPRs {k.get('TotalSGPRs'):>3s}  LDS {k.get('LDS'):>5s} B  scratch {k.get('ScratchSize')}  "
            f"waves/SIMD {k.get('Occupancy')}")


def regs_section(a):
    from as_cops_and_thieves_amd import _learn_native as ln
    out = ["", "## 2. registers, LDS and scratch of csrc/cat_ppo.hip: the loss, gradient-norm and Adam kernels (by value and _dev) and the schedule kernel",
           "#    (hipcc " + " ".join(f for f in ln.HIPCC_FLAGS if f not in ("-fPIC", "-shared")) + " -Rpass-analysis=kernel-resource-usage)", "this commit:"]
    now = kernel_resources(ln.PKG / "csrc" / "cat_ppo.hip", ln.ROOT / "include")
    out += [_row(n, k) for n, k in now.items()]
    new = {n: k for n, k in now.items() if "_dev" in n or "schedule_kernel" in n}
    out.append(f"scratch of the {len(new)} new kernels: " + ("none" if all(k.get("ScratchSize") == "0" for k in new.values()) else "SOME -- see above"))
    if not a.parent_src:
        return out + ["parent commit: not taken (--parent-src FILE --parent-include DIR)"]
    before = kernel_resources(a.parent_src, a.parent_include or ln.ROOT / "include")
    out += ["parent commit (the three kernels before they became templates):"] + [_row(n, k) for n, k in before.items()]
    for want in KERNELS[:3]:
        (old,) = [k for n, k in before.items() if want in n]
        (cur,) = [k for n, k in now.items() if want in n and "_dev" not in n]
        same = all(old.get(f) == cur.get(f) for f in ("VGPRs", "TotalSGPRs", "ScratchSize"))
        out.append(f"{want} by value: VGPRs / SGPRs / scratch {cur.get('VGPRs')} / {cur.get('TotalSGPRs')} / {cur.get('ScratchSize')} against the parent's "
                   f"{old.get('VGPRs')} / {old.get('TotalSGPRs')} / {old.get('ScratchSize')}: {'EQUAL' if same else 'DIFFERENT'}")
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hyper_schedule.txt"))
    a = ap.parse_args()
    if not a.regs_only and not torch.cuda.is_available():
        sys.exit("hyper_schedule_bench: no GPU; no speed is measured without one (--regs-only: the compiler's figures alone)")
    lines = [f"# learner schedules on the device (RoleConfig.lr_schedule) against the learner without them; env-core source {source_sha16()}; "
             + ("no device" if a.regs_only else torch.cuda.get_device_name(0))]
    lines += (["## 1. speed", "not taken (--regs-only)"] if a.regs_only else speed_section(a)) + regs_section(a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
