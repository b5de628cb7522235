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
import option_cost


def main():
    a = option_cost.parse([("--lanes", dict(default="64,256,1024")), ("--horizon", dict(type=int, default=64)),
                           ("--samples", dict(type=int, default=256)), ("--bc-weight", dict(type=float, default=1.0))],
                          help="off or labels-L")
    on = a.leg != "off"

    def options():
        if not on:
            return {}
        from ddpg_trucktrailer_amd.demo_loss import DemoLoss
        from ddpg_trucktrailer_amd.mpc import ExpertLabels, MPCConfig
        return {"labels": ExpertLabels(int(a.leg.split("-")[1]), MPCConfig(horizon=a.horizon, samples=a.samples), seed=27),
                "demo_loss": DemoLoss(a.bc_weight, q_filter=False)}

    if a.leg:
        return option_cost.one_leg(a, options, stats=(lambda loop: f" demo_stats={loop.demo_stats()}") if on else None)
    with_labels = [f"labels-{int(x)}" for x in a.lanes.split(",") if x]
    names = {v: f"ExpertLabels({v.split('-')[1]}, H = {a.horizon}, S = {a.samples}) + DemoLoss({a.bc_weight}, no filter)" for v in with_labels}
    option_cost.compare(a, __file__, ["off"] + with_labels, ["--horizon", str(a.horizon), "--samples", str(a.samples), "--bc-weight", str(a.bc_weight)],
                        {"off": "the loop without labels", **names}, 68, records=True)


if __name__ == "__main__":
    main()
