#!/usr/bin/env python3
"""GPU: what a gradient clip costs in the loop, and that a loop without one costs what the parent commit's does.

ms per vector step of DDPGRollout at N = 4096 envs, 64 updates per step, B = 256, graph-replayed (the configuration whose step time
is the learn chain's latency): `legs` legs each of the loop without a clip ("off"), with GradClip(--critic, --actor) ("on": the
separate-optimizer order, nine launches per update; a value <= 0 leaves that network without a clip) and,
with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's loop ("parent").  Every leg is a fresh
process; the variants alternate within a round and their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the leg without a clip: its median at most the parent's median plus the parent legs'
own max - min (it launches the parent's kernels: anything else is a host-side regression).  on - off is a record, not a gate.
Usage: grad_clip_cost.py [--legs 3] [--steps 400] [--warmup 60] [--critic 1e4] [--actor 1.0] [--parent-tree DIR] [--out FILE]
       grad_clip_cost.py --leg off|on [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, UPD, B, SLOTS, GRAPH_STEPS = 4096, 64, 256, 64, 4


def one_leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    kw = {}
    if a.leg == "on":
        from ddpg_trucktrailer_amd.grad_clip import GradClip
        kw["grad_clip"] = GradClip(a.critic if a.critic > 0 else None, a.actor if a.actor > 0 else None)
    env = TruckTrailerVecEnv(N)
    env.reset(seed=27)
    loop = DDPGRollout(env, batch_size=B, replay_slots=SLOTS, seed=27, updates_per_step=UPD, graph_steps=GRAPH_STEPS, **kw)
    loop.run(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(a.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    assert loop.graph_steps == GRAPH_STEPS and loop.handover_gave_up == [] and loop.learner.tail_gave_up() == 0
    assert all(torch.isfinite(p).all() for p in loop.agent.actor.parameters())
    print(f"pipeline={loop.pipeline} fuse_tail={loop.learner.fuse_tail} updates={int(loop.learner.step_dev.item())}")
    if a.leg == "on":
        print("CLIP " + "; ".join(f"{k}: clipped {v['clipped']} of {v['updates']}, last norm {v['norm']:.4g}" for k, v in loop.learner.clip_stats().items()))
    print(f"LEG {ms:.5f}")


def run_leg(a, variant):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "off" if variant == "parent" else variant, "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--critic", str(a.critic), "--actor", str(a.actor)]
    if variant == "parent":
        cmd += ["--tree", a.parent_tree]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    for ln in out.splitlines():
        if ln.startswith("CLIP "):
            print("      " + ln, flush=True)
    return float([ln for ln in out.splitlines() if ln.startswith("LEG ")][-1].split()[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--critic", type=float, default=1e4)
    ap.add_argument("--actor", type=float, default=1.0)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("off", "on"), default=None)
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    if a.leg:
        return one_leg(a)
    variants = ["off", "on"] + (["parent"] if a.parent_tree else [])
    res = {v: [] for v in variants}
    for leg in range(a.legs):
        for v in (variants if leg % 2 == 0 else variants[::-1]):
            res[v].append(run_leg(a, v))
            print(f"round {leg} {v:>6}: {res[v][-1]:.5f} ms per vector step", flush=True)
    names = dict(off="the loop without a clip", on=f"GradClip({a.critic if a.critic > 0 else None}, {a.actor if a.actor > 0 else None})",
                 parent="the parent commit's loop")
    lines = [f"# DDPGRollout, N = {N}, {UPD} updates per vector step, B = {B}, ring of {SLOTS} slots, whole-step graphs of {GRAPH_STEPS}; "
             f"{a.steps} timed vector steps per leg after {a.warmup}, every leg a fresh process, {a.legs} legs, variants alternating"]
    for v in variants:
        x = res[v]
        lines.append(f"{names[v]:>28}: " + "  ".join(f"leg {i} {t:8.5f}" for i, t in enumerate(x)) +
                     f"  | median {statistics.median(x):8.5f} ms per vector step, max - min {max(x) - min(x):7.5f}")
    off, on = statistics.median(res["off"]), statistics.median(res["on"])
    spread = max(res["off"]) - min(res["off"])
    lines.append(f"# on - off = {1e3 * (on - off):+.2f} us per vector step = {1e3 * (on - off) / UPD:+.3f} us per update; the off legs' own max - min "
                 f"is {1e3 * spread:.2f} us per vector step: " + ("within it" if on - off <= spread else "beyond it"))
    if a.parent_tree:
        p = res["parent"]
        limit = statistics.median(p) + (max(p) - min(p))
        lines.append(f"# gate: off median {off:.5f} ms against the parent's median + its legs' max - min = {limit:.5f} ms: "
                     + ("within" if off <= limit else "NOT within"))
    else:
        lines.append("# no --parent-tree: the gate against the parent commit was not evaluated")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
