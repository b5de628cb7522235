#!/usr/bin/env python3
"""GPU: what a TD3 update costs beside a DDPG update.

us per graph-replayed update at B = 256, `updates` updates per leg: the lone FusedLearner with the tail in one launch (the yardstick:
its code objects are the parent's), TD3 at policy_delay 1 (every update full) and TD3 at policy_delay 2 (critic-only and full updates
in alternation: the average update).  `legs` legs of each, the three variants alternating within a leg and their order from leg
to leg, in one process.  Every leg is printed, and written to --out.  The rule of DESIGN.md section 13: is the delay-2 median within
the DDPG median plus the DDPG legs' own max - min?
Usage: td3_cost.py [--legs 3] [--updates 1000] [--per-graph 8] [--out profiles/td3_cost.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ddpg_trucktrailer_amd.agent import Agent  # noqa: E402
from ddpg_trucktrailer_amd.fused_learn import FusedLearner  # noqa: E402
from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing  # noqa: E402
from ddpg_trucktrailer_amd.rollout import _CAPTURE_MODE, _SEED_STRIDE  # noqa: E402
from ddpg_trucktrailer_amd.td3 import TD3Config, TD3Learner  # noqa: E402

DEV = torch.device("cuda:0")
B = 256


def ring(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = TrajectoryRing(2048, 16, 23, DEV)
    r.obs.copy_(torch.rand(r.obs.shape, device=DEV, generator=g) * 2 - 1)
    r.act.copy_(torch.rand(r.act.shape, device=DEV, generator=g) * 2 - 1)
    r.rew.copy_(torch.rand(r.rew.shape, device=DEV, generator=g) * 10 - 5)
    r.done.copy_((torch.rand(r.done.shape, device=DEV, generator=g) < 0.05).to(torch.uint8))
    r.k = 15
    r.k_dev.fill_(15)
    return r


def agent(seed, td3=None):
    torch.manual_seed(seed)
    return Agent(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=B, device=DEV, replay=False, td3=td3)


def ddpg_update():
    rg, fl = ring(200), FusedLearner(agent(100), B)
    fl.fuse_tail = True
    bufs = rg._batch_bufs(B)[:5]

    def update(u):
        fl.learn_batch(*bufs, sample=rg.sample_args(B, seed=(300 + u * _SEED_STRIDE) & (2 ** 64 - 1)))
    return fl, update


def td3_update(delay):
    fl = TD3Learner(agent(100, TD3Config(policy_delay=delay)), B, ring(200), 300)
    return fl, lambda u: fl.learn_batch(u=u, full=(u + 1) % delay == 0)


def captured(fn, per_graph):
    for u in range(4):
        fn(u)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode=_CAPTURE_MODE):
        for u in range(per_graph):
            fn(u)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g


def timed(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--updates", type=int, default=1000)
    ap.add_argument("--per-graph", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.per_graph % 2 == 0, "an even number of updates per graph: as many full as critic-only ones at delay 2"
    replays = max(1, -(-a.updates // a.per_graph))
    variants = [("DDPG (lone FusedLearner, tail in one launch)", ddpg_update), ("TD3, policy_delay 1", lambda: td3_update(1)),
                ("TD3, policy_delay 2", lambda: td3_update(2))]
    made = {}
    for name, make in variants:
        fl, fn = make()
        made[name] = (fl, captured(fn, a.per_graph))
    res = {name: [] for name, _ in variants}
    for leg in range(a.legs):
        for name, _ in (variants if leg % 2 == 0 else variants[::-1]):
            res[name].append(timed(made[name][1], replays) / (replays * a.per_graph))
    lines = [f"# learn() alone, B = {B}, {replays * a.per_graph} graph-replayed updates per leg ({a.per_graph} per graph), {a.legs} legs, variants "
             "alternating, ring of 16 slots x 2048 envs, 5 % done flags",
             f"# device {torch.cuda.get_device_name(0)}"]
    for name, _ in variants:
        assert made[name][0].tail_gave_up() == 0
        x = res[name]
        lines.append(f"{name:>46}: " + "  ".join(f"leg {i} {v:7.2f}" for i, v in enumerate(x)) +
                     f"  | median {statistics.median(x):7.2f} us per update, max - min {max(x) - min(x):5.2f}")
    ddpg, td3 = res[variants[0][0]], res[variants[2][0]]
    limit = statistics.median(ddpg) + (max(ddpg) - min(ddpg))
    lines.append(f"# delay-2 median {statistics.median(td3):.2f} us against the DDPG median + the DDPG legs' max - min = {limit:.2f} us: "
                 + ("within" if statistics.median(td3) <= limit else "NOT within"))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
