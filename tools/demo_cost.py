#!/usr/bin/env python3
"""GPU: what the demonstration loss costs in the loop, and that a loop without one costs what the parent commit's does (DESIGN.md
section 25).

ms per vector step of DDPGRollout at N = 4096 envs, 64 updates per step, B = 256, graph-replayed (the configuration whose step time
is the learn chain's latency): `legs` legs each of the loop without the option ("off"), with DemoLoss(--bc-weight) and a side buffer of
a quarter of the ring's transitions ("on") and, with --parent-tree DIR (a checkout of the parent commit with its library built), the
parent's loop ("parent").  Every leg is a fresh process; the variants alternate within a round and their order from round to round.
Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the leg without the option: its median at most the parent's median plus the parent
legs' own max - min (it launches the parent's kernels: anything else is a regression in shared code).  on - off is a record, not a
gate: the "on" loop also draws a quarter of its rows from the side buffer, which the "off" loop does not have.
Usage: demo_cost.py [--legs 3] [--steps 400] [--warmup 60] [--bc-weight 1.0] [--no-q-filter] [--parent-tree DIR] [--out FILE]
       demo_cost.py --leg off|on [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, UPD, B, SLOTS, GRAPH_STEPS = 4096, 64, 256, 64, 4
SIDE = SLOTS * N // 4


def one_leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    kw = {}
    if a.leg == "on":
        from ddpg_trucktrailer_amd.demo_loss import DemoLoss
        kw["demo_loss"] = DemoLoss(a.bc_weight, not a.no_q_filter)
    env = TruckTrailerVecEnv(N)
    env.reset(seed=27)
    loop = DDPGRollout(env, batch_size=B, replay_slots=SLOTS, seed=27, updates_per_step=UPD, graph_steps=GRAPH_STEPS, **kw)
    if a.leg == "on":
        g = torch.Generator().manual_seed(5)
        loop.ring.load_side(torch.rand((SIDE, 23), generator=g) * 2 - 1, torch.rand(SIDE, generator=g) * 2 - 1, torch.randn(SIDE, generator=g),
                            torch.rand((SIDE, 23), generator=g) * 2 - 1, (torch.rand(SIDE, generator=g) < 0.05).to(torch.uint8))
    loop.run(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(a.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    assert loop.graph_steps == GRAPH_STEPS and loop.handover_gave_up == [] and loop.learner.tail_gave_up() == 0
    assert all(torch.isfinite(p).all() for p in loop.agent.actor.parameters())
    print(f"pipeline={loop.pipeline} fuse_tail={loop.learner.fuse_tail} updates={int(loop.learner.step_dev.item())}" +
          (f" demo_stats={loop.demo_stats()}" if a.leg == "on" else ""))
    print(f"LEG {ms:.5f}")


def run_leg(a, variant):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "off" if variant == "parent" else variant, "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--bc-weight", str(a.bc_weight)] + (["--no-q-filter"] if a.no_q_filter else [])
    if variant == "parent":
        cmd += ["--tree", a.parent_tree]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return float([ln for ln in out.splitlines() if ln.startswith("LEG ")][-1].split()[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--bc-weight", type=float, default=1.0)
    ap.add_argument("--no-q-filter", action="store_true")
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
    names = dict(off="the loop without demo_loss", on=f"DemoLoss({a.bc_weight}, {not a.no_q_filter}), {SIDE} side tuples",
                 parent="the parent commit's loop")
    lines = [f"# DDPGRollout, N = {N}, {UPD} updates per vector step, B = {B}, ring of {SLOTS} slots, whole-step graphs of {GRAPH_STEPS}; "
             f"{a.steps} timed vector steps per leg after {a.warmup}, every leg a fresh process, {a.legs} legs, variants alternating"]
    for v in variants:
        x = res[v]
        lines.append(f"{names[v]:>40}: " + "  ".join(f"leg {i} {t:8.5f}" for i, t in enumerate(x)) +
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
