#!/usr/bin/env python3
"""GPU: what expert labels cost in the loop, and that a loop without them costs what the parent commit's does.

ms per vector step of DDPGRollout at N = 4096 envs, 64 updates per step, B = 256, graph-replayed (the configuration whose step time
is the learn chain's latency): `legs` legs each of the loop without the option ("off"), with ExpertLabels(L, H = 64, S = 256) and
DemoLoss(--bc-weight, q_filter=False) for each L of --lanes ("labels-L") and, with --parent-tree DIR (a checkout of the parent commit
with its library built), the parent's loop ("parent").  Every leg is a fresh process; the variants alternate within a round and
their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the leg without the option: its median at most the parent's median plus the parent
legs' own max - min (it launches the parent's kernels).  The legs with labels are records, not gates: ms per step over the off leg.
The new launch's own average time comes from a kernel trace of one leg, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/expert_labels_cost.py --leg labels-256
Usage: expert_labels_cost.py [--legs 3] [--steps 400] [--warmup 60] [--lanes 64,256,1024] [--horizon 64] [--samples 256]
                             [--bc-weight 1.0] [--parent-tree DIR] [--out FILE]
       expert_labels_cost.py --leg off|labels-L [--tree DIR] ...   (one leg in this process; prints "LEG <ms per vector step>")"""
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
    if a.leg != "off":
        from ddpg_trucktrailer_amd.demo_loss import DemoLoss
        from ddpg_trucktrailer_amd.mpc import ExpertLabels, MPCConfig
        kw["labels"] = ExpertLabels(int(a.leg.split("-")[1]), MPCConfig(horizon=a.horizon, samples=a.samples), seed=27)
        kw["demo_loss"] = DemoLoss(a.bc_weight, q_filter=False)
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
    print(f"pipeline={loop.pipeline} fuse_tail={loop.learner.fuse_tail} updates={int(loop.learner.step_dev.item())}" +
          (f" demo_stats={loop.demo_stats()}" if a.leg != "off" else ""))
    print(f"LEG {ms:.5f}")


def run_leg(a, variant):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "off" if variant == "parent" else variant, "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--horizon", str(a.horizon), "--samples", str(a.samples),
           "--bc-weight", str(a.bc_weight)]
    if variant == "parent":
        cmd += ["--tree", a.parent_tree]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return float([ln for ln in out.splitlines() if ln.startswith("LEG ")][-1].split()[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--lanes", default="64,256,1024")
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--bc-weight", type=float, default=1.0)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="off or labels-L")
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    if a.leg:
        return one_leg(a)
    with_labels = [f"labels-{int(x)}" for x in a.lanes.split(",") if x]
    variants = (["parent"] if a.parent_tree else []) + ["off"] + with_labels
    res = {v: [] for v in variants}
    for leg in range(a.legs):
        for v in (variants if leg % 2 == 0 else variants[::-1]):
            res[v].append(run_leg(a, v))
            print(f"round {leg} {v:>9}: {res[v][-1]:.5f} ms per vector step", flush=True)
    names = {"off": "the loop without labels", "parent": "the parent commit's loop"}
    for v in with_labels:
        names[v] = f"ExpertLabels({v.split('-')[1]}, H = {a.horizon}, S = {a.samples}) + DemoLoss({a.bc_weight}, no filter)"
    lines = [f"# DDPGRollout, N = {N}, {UPD} updates per vector step, B = {B}, ring of {SLOTS} slots, whole-step graphs of {GRAPH_STEPS}; "
             f"{a.steps} timed vector steps per leg after {a.warmup}, every leg a fresh process, {a.legs} legs, variants alternating"]
    for v in variants:
        x = res[v]
        lines.append(f"{names[v]:>68}: " + "  ".join(f"leg {i} {t:8.5f}" for i, t in enumerate(x)) +
                     f"  | median {statistics.median(x):8.5f} ms per vector step, max - min {max(x) - min(x):7.5f}")
    off = statistics.median(res["off"])
    spread = max(res["off"]) - min(res["off"])
    for v in with_labels:
        on = statistics.median(res[v])
        lines.append(f"# {v} - off = {1e3 * (on - off):+.2f} us per vector step ({100 * (on - off) / off:+.2f} %); the off legs' own max - min is "
                     f"{1e3 * spread:.2f} us per vector step (a record, not a gate)")
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
