#!/usr/bin/env python3
"""What end-of-episode positions cost: the one more pointer in the env kernels' launch arguments, and the store when a buffer is bound.

    python tools/final_positions_bench.py timing --parent-lib PARENT/as_cops_and_thieves_amd/libcat_sim.so [--reps 7] [--out profiles/final_positions.txt]
    python tools/final_positions_bench.py resources --parent-src PARENT [--out profiles/final_positions.txt]

PARENT is a checkout of the parent commit (``git worktree add PARENT HEAD~1``), built there for ``timing``.

``timing`` (needs a GPU): bench.py's default leg -- labyrinth 2v1 x 4096 envs, 64 rays, 600 burn-in ticks, 200 warm-up and 2000 timed one-tick
launches (``bench.timed_steps``), then the resident launch at T = 64 (``bench.timed_rollout``) -- in three configurations: the parent commit's
library (``CAT_SIM_LIB``), this tree's with nothing bound, this tree's with a buffer bound ([N, A, 2], and [T, N, A, 2] for the resident
launch).  Every measurement is a process of its own; the configurations alternate, in an order that rotates and reverses from repetition to
repetition, at least 6 repetitions each.  THE CONDITION: the unbound median lies inside the parent's own range (min .. max) of this session.
The verdict is written out either way.

``resources`` (no GPU): ``-Rpass-analysis=kernel-resource-usage`` of the env core's translation unit, this tree against PARENT, for the four
env kernels (step_kernel, step_kernel_pooled, rollout_kernel, rollout_kernel_pooled) in every instantiation.  THE CONDITION: no kernel gains
scratch.

Each mode rewrites its own section of the output file and keeps the other's.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CONFIGS = ("parent", "unbound", "bound")
ENV_KERNELS = ("step_kernel", "step_kernel_pooled", "rollout_kernel", "rollout_kernel_pooled")


def worker(bound: bool, steps: int, warmup: int, T: int) -> None:
    """One measurement in this process: prints one JSON line."""
    import torch
    import bench
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    fence = lambda: torch.cuda.synchronize(dev)
    hip = bench.HipEvents()
    sim, cfg, _ = bench.build_sim("labyrinth", 2, 1, 4096, 64, 0, dev)
    sim.reset()
    for t in range(600):
        sim.step_fused(None, tick=t, auto_reset=True)
    if bound:
        one = torch.full((cfg.n_envs, cfg.n_agents, 2), 0x7E00, dtype=torch.int16, device=dev).view(torch.float16)
        sim.bind_final_positions(one)
    elapsed, tick_ms, _, _ = bench.timed_steps(sim, steps, warmup, fence, hip, first_tick=600)
    if bound:
        rows = torch.full((T, cfg.n_envs, cfg.n_agents, 2), 0x7E00, dtype=torch.int16, device=dev).view(torch.float16)
        sim.bind_final_positions(rows)
    _, roll_ms, _ = bench.timed_rollout(sim, T, fence, hip, first_tick=600 + warmup + steps)
    written = None
    if bound:
        fence()
        written = int((rows.view(torch.int16) != 0x7E00).any(-1).any(-1).sum())
    assert sim.device_errors() == 0
    print(json.dumps({"env_steps_per_s": cfg.n_envs * steps / elapsed, "one_tick_kernel_us": 1e3 * tick_ms, "resident_us_per_tick": 1e3 * roll_ms,
                      "kernel": sim.one_tick_kernel, "rows_written": written}), flush=True)


def timing(args) -> list:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("final_positions_bench timing needs a GPU")
    parent = Path(args.parent_lib).resolve()
    if not parent.exists():
        raise SystemExit(f"--parent-lib {parent} does not exist: build the parent commit's checkout first")
    reps = max(6, args.reps)
    got = {c: [] for c in CONFIGS}
    for r in range(reps):
        order = list(CONFIGS[r % 3:] + CONFIGS[:r % 3])
        if r % 2:
            order.reverse()
        for c in order:
            env = dict(os.environ)
            env.pop("CAT_SIM_LIB", None)
            if c == "parent":
                env["CAT_SIM_LIB"] = str(parent)
            cmd = [sys.executable, str(Path(__file__).resolve()), "worker", "--steps", str(args.steps), "--warmup", str(args.warmup), "--T", str(args.T)]
            res = subprocess.run(cmd + (["--bound"] if c == "bound" else []), env=env, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(f"worker {c} failed ({res.returncode}):\n{res.stderr[-2000:]}")
            got[c].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"[rep {r} {c}] {got[c][-1]}", flush=True)
    lines = [f"labyrinth 2v1 x 4096 envs, 64 rays; {torch.cuda.get_device_name(0)}; {reps} repetitions per configuration, one process each, order: "
             "parent / unbound / bound rotated by one and reversed every other repetition",
             f"one-tick: {args.warmup} warm-up + {args.steps} timed cat_step_fused launches; resident: cat_rollout_fused T = {args.T}, 4 timed launches",
             f"one-tick kernel: {got['unbound'][0]['kernel']}", ""]
    verdicts = []
    for key, what in (("env_steps_per_s", "one-tick env-steps/s (wall clock of the timed region; bench.py's `value`)"),
                      ("one_tick_kernel_us", "one-tick kernel, us per launch (events attached to the dispatch)"),
                      ("resident_us_per_tick", "resident launch, kernel us per tick")):
        lines.append(what)
        stat = {}
        for c in CONFIGS:
            v = [m[key] for m in got[c]]
            stat[c] = (statistics.median(v), min(v), max(v))
            lines.append(f"  {c:8s} median {stat[c][0]:12.3f}  min {stat[c][1]:12.3f}  max {stat[c][2]:12.3f}   all: " + " ".join(f"{x:.3f}" for x in v))
        inside = stat["parent"][1] <= stat["unbound"][0] <= stat["parent"][2]
        verdicts.append(inside)
        lines.append(f"  unbound median / parent median = {stat['unbound'][0] / stat['parent'][0]:.4f}; bound median / unbound median = "
                     f"{stat['bound'][0] / stat['unbound'][0]:.4f}")
        lines.append(f"  CONDITION (unbound median inside the parent's range {stat['parent'][1]:.3f} .. {stat['parent'][2]:.3f}): "
                     + ("MET" if inside else "NOT MET"))
        lines.append("")
    lines.append(f"rows a bound resident launch wrote (of {args.T} x 4096): " + " ".join(str(m["rows_written"]) for m in got["bound"]))
    lines.append("OVERALL: " + ("the unbound figures lie inside the parent's run-to-run range" if all(verdicts) else
                                "NOT every unbound figure lies inside the parent's run-to-run range (see above)"))
    return lines


def parse_remarks(text: str) -> dict:
    """mangled kernel name -> {sgpr, vgpr, scratch, sgpr_spill, vgpr_spill, occupancy} from hipcc's kernel-resource-usage remarks."""
    fields = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
              "Occupancy [waves/SIMD]": "occupancy"}
    table, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            table[name] = {}
            continue
        for label, key in fields.items():
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and name is not None:
                table[name][key] = int(m.group(1))
    return table


def resource_table(src_root: Path) -> dict:
    from as_cops_and_thieves_amd import _native as nat
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *nat.HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", f"-I{src_root / 'include'}", "-o", os.devnull,
           str(src_root / "as_cops_and_thieves_amd" / "csrc" / "cat_sim.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise SystemExit(f"hipcc failed on {src_root}:\n{res.stderr[-2000:]}")
    return parse_remarks(res.stderr)


def short_name(mangled: str) -> str:
    """``step_kernel_pooled<FixDims<3,64,2>, fan 1, exact 0>`` from the mangled name of an env kernel; "" for anything else."""
    m = re.search(r"\d+(step_kernel_pooled|rollout_kernel_pooled|step_kernel|rollout_kernel)INS_7WithFanINS_\d(TreeDims|DynDims|FixDims)(.*?)EvPKNS_6Params", mangled)
    if not m:
        return ""
    kernel, dims, rest = m.groups()
    if dims == "FixDims":
        dims = "FixDims<" + ",".join(re.findall(r"Li(\d+)E", rest)[:3]) + ">"
    fan = re.findall(r"Li(\d+)E", rest)[-1]
    flag = re.search(r"Lb(\d)E", rest)
    return f"{kernel}<{dims}, fan {fan}" + (f", exact {flag.group(1)}" if flag else "") + ">"


def resources(args) -> list:
    parent = Path(args.parent_src).resolve()
    new, old = resource_table(ROOT), resource_table(parent)
    lines = ["env kernels, hipcc -Rpass-analysis=kernel-resource-usage (gfx950): this tree / parent",
             f"  {'kernel instantiation':70s} {'SGPR':>9s} {'VGPR':>9s} {'scratch':>9s} {'SGPR spill':>11s} {'VGPR spill':>11s} {'occ':>5s}"]
    worse = []
    for name in sorted(new, key=lambda n: (short_name(n), n)):
        sn = short_name(name)
        if not sn or sn.split("<")[0] not in ENV_KERNELS:
            continue
        a, b = new[name], old.get(name)
        if b is None:
            lines.append(f"  {sn:70s} (no such kernel in the parent)")
            worse.append(sn)
            continue
        cell = lambda k: f"{a[k]}/{b[k]}"
        lines.append(f"  {sn:70s} {cell('sgpr'):>9s} {cell('vgpr'):>9s} {cell('scratch'):>9s} {cell('sgpr_spill'):>11s} {cell('vgpr_spill'):>11s} {cell('occupancy'):>5s}")
        if a["scratch"] > b["scratch"]:
            worse.append(sn)
    lines.append("CONDITION (no kernel gains scratch): " + ("MET" if not worse else "NOT MET: " + ", ".join(worse)))
    return lines


def write_section(out: Path, section: str, lines: list) -> None:
    """Replace ``[section]`` of the file (up to the next ``[...]`` header or the end), keep everything else."""
    text = out.read_text() if out.exists() else ""
    parts = re.split(r"(?m)^(?=\[[a-z]+\]$)", text)
    parts = [p for p in parts if p.strip() and not p.startswith(f"[{section}]")]
    parts.append(f"[{section}]\n" + "\n".join(lines) + "\n\n")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(sorted(parts, key=lambda p: 0 if p.startswith("[timing]") else 1)))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("timing", "resources", "worker"))
    ap.add_argument("--parent-lib", type=Path, help="timing: libcat_sim.so built from the parent commit")
    ap.add_argument("--parent-src", type=Path, help="resources: a checkout of the parent commit")
    ap.add_argument("--reps", type=int, default=7, help="repetitions per configuration (at least 6)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--bound", action="store_true", help="worker: bind a buffer")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "final_positions.txt")
    args = ap.parse_args()
    if args.mode == "worker":
        worker(args.bound, args.steps, args.warmup, args.T)
        return 0
    if args.mode == "timing" and args.parent_lib is None or args.mode == "resources" and args.parent_src is None:
        ap.error("timing needs --parent-lib, resources needs --parent-src")
    lines = timing(args) if args.mode == "timing" else resources(args)
    print("\n".join(lines))
    write_section(args.out, args.mode, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
