#!/usr/bin/env python3
"""GPU: what one greedy evaluation costs, as a record, not a gate.

One evaluation of K = 4 agents x 4096 lanes (evaluation.Evaluator; untrained reference-shaped actors, seeds 0..3; start poses
from seed 0) in three forms: "graph" (a hipGraph of 32 steps per replay, one look per replay), "eager" (the same launches one by
one) and "host" (grid_eval's host-masked loop: the plain step with info, a torch `where` chain and a synchronize per step).  Every
leg is a fresh process that runs the evaluation twice and times the second run; `legs` legs per form, the forms alternating.
Reported per form: wall time, steps run, and the share of the step launches in which more than half the workgroups were wholly
held (from the records' lengths: lane i is live in launch t <=> len[i] >= t).
--trace: additionally two runs under `rocprofv3 --kernel-trace --stats`, each in a process of its own -- the eager evaluation
(k_step_hold) and the same number of plain steps of an env of the same N with the same actors (k_step) -- and the average
duration of each kernel.
Usage: eval_cost.py [--legs 3] [--trace] [--out FILE]
       eval_cost.py --leg graph|eager|host|plain"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, LANES, CHUNK, BLOCK = 4, 4096, 32, 256


def _actors(dev):
    import torch
    from ddpg_trucktrailer_amd.networks import ActorNetwork
    out = []
    for a in range(K):
        torch.manual_seed(a)
        out.append(ActorNetwork(1e-4, (23,), 400, 300, 1, name=f"actor{a}", device=dev))
    return out


def one_leg(form):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from ddpg_trucktrailer_amd import fused
    from ddpg_trucktrailer_amd.evaluation import Evaluator
    dev = torch.device("cuda:0")
    actors = _actors(dev)
    ev = Evaluator(LANES, agents=K, seed=0, chunk=CHUNK, device=dev, use_graph=form == "graph")
    if form == "plain":      # the plain step at the same N, for the kernel trace: as many launches as the evaluation's longest episode
        from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
        steps = int(max(int(r["len"].max()) for r in ev.run(actors)))
        env = TruckTrailerVecEnv(K * LANES, device=dev)
        env.set_pose(ev._start)
        mu = torch.zeros(K * LANES, dtype=torch.float32, device=dev)
        for _ in range(steps):
            for a, net in enumerate(actors):
                fused.actor_forward(net, env.obs[a * LANES:(a + 1) * LANES], mu[a * LANES:(a + 1) * LANES])
            env.step(mu * ev.high, auto_reset=False)
        torch.cuda.synchronize()
        print("LEG " + json.dumps({"form": form, "steps": steps}))
        return
    host = form == "host"
    ev.run(actors, host_loop=host)               # (captures, allocations, first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = ev.run(actors, host_loop=host)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    length = torch.cat([r["len"] for r in recs]).cpu().numpy()
    longest = length.reshape(-1, BLOCK).max(axis=1)                 # a workgroup is live in launches 1 .. its longest episode
    launches = ev.steps_run
    held_share = [(longest < t).mean() for t in range(1, launches + 1)]
    print("LEG " + json.dumps({"form": form, "wall_ms": wall * 1e3, "steps": launches, "longest_episode": int(length.max()),
                               "mostly_held_launches": float(np.mean([h > 0.5 for h in held_share])),
                               "mean_return": float(torch.cat([r["ret"] for r in recs]).mean())}))


def run_leg(form):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", form], check=True, capture_output=True, text=True,
                         timeout=600).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("LEG ")][-1][4:])


def trace(form, kernel):
    """Average duration (us) and calls of the kernels named like `kernel` in a rocprofv3 kernel trace of one leg."""
    d = tempfile.mkdtemp(prefix="eval_cost_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--",
                        sys.executable, os.path.abspath(__file__), "--leg", form], check=True, capture_output=True, text=True, timeout=900)
        calls, total = 0, 0.0
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if kernel in row["Name"]:
                    calls += int(row["Calls"])
                    total += float(row["TotalDurationNs"])
        return (total / calls / 1e3 if calls else float("nan")), calls
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("graph", "eager", "host", "plain"), default=None)
    a = ap.parse_args()
    if a.leg:
        return one_leg(a.leg)
    forms = ["graph", "eager", "host"]
    res = {f: [] for f in forms}
    for leg in range(a.legs):
        for f in (forms if leg % 2 == 0 else forms[::-1]):
            res[f].append(run_leg(f))
            print(f"round {leg} {f:>6}: {res[f][-1]}", flush=True)
    lines = [f"# one evaluation of K = {K} agents x {LANES} lanes (untrained actors), chunk {CHUNK}; the second run() of a fresh process, "
             f"{a.legs} legs per form, forms alternating"]
    for f in forms:
        x = [r["wall_ms"] for r in res[f]]
        r = res[f][0]
        lines.append(f"{f:>6}: " + "  ".join(f"leg {i} {t:9.2f}" for i, t in enumerate(x)) + f"  | median {statistics.median(x):9.2f} ms, "
                     f"{r['steps']} step launches (longest episode {r['longest_episode']}), more than half the workgroups held in "
                     f"{100 * r['mostly_held_launches']:.1f} % of them")
    same = len({json.dumps(r["mean_return"]) for f in forms for r in res[f]}) == 1
    lines.append(f"# mean return of all legs: {res['graph'][0]['mean_return']!r}" + (" (the same bits in every leg)" if same else " (legs DIFFER)"))
    if a.trace:
        hold, n_hold = trace("eager", "k_step_hold")
        plain, n_plain = trace("plain", "::k_step<")
        lines.append(f"# rocprofv3 --kernel-trace --stats, a run each: k_step_hold {hold:.2f} us average over {n_hold} launches (held lanes and "
                     f"workgroups included), k_step {plain:.2f} us average over {n_plain} launches at the same N = {K * LANES}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
