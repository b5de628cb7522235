#!/usr/bin/env python3
"""GPU: what expert lanes cost in the loop, and that a loop without them costs what the parent commit's does.

ms per vector step of DDPGRollout at N = 4096 envs, 64 updates per step, B = 256, graph-replayed (the configuration whose step time
is the learn chain's latency): `legs` legs each of the loop without the option ("off"), with ExpertLanes(64, H = 64, S = 256) acting
only ("expert"), with the same lanes and DemoLoss(--bc-weight) ("expert+bc") and, with --parent-tree DIR (a checkout of the parent
commit with its library built), the parent's loop ("parent").  Every leg is a fresh process; the variants alternate within a round
and their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the leg without the option: its median at most the parent's median plus the parent
legs' own max - min (it launches the parent's kernels).  The legs with expert lanes are records, not gates: ms per step over the off
leg.  The new launch's own average time comes from a kernel trace of one leg, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/expert_lanes_cost.py --leg expert
Usage: expert_lanes_cost.py [--legs 3] [--steps 400] [--warmup 60] [--lanes 64] [--horizon 64] [--samples 256] [--bc-weight 1.0]
                            [--parent-tree DIR] [--out FILE]
       expert_lanes_cost.py --leg off|expert|expert+bc [--tree DIR] ...   (one leg in this process; prints "LEG <ms per vector step>")"""
import option_cost


def main():
    a = option_cost.parse([("--lanes", dict(type=int, default=64)), ("--horizon", dict(type=int, default=64)),
                           ("--samples", dict(type=int, default=256)), ("--bc-weight", dict(type=float, default=1.0))],
                          choices=("off", "expert", "expert+bc"))
    bc = a.leg == "expert+bc"

    def options():
        kw = {}
        if a.leg != "off":
            from ddpg_trucktrailer_amd.mpc import ExpertLanes, MPCConfig
            kw["expert"] = ExpertLanes(a.lanes, MPCConfig(horizon=a.horizon, samples=a.samples), seed=27)
        if bc:
            from ddpg_trucktrailer_amd.demo_loss import DemoLoss
            kw["demo_loss"] = DemoLoss(a.bc_weight)
        return kw

    if a.leg:
        return option_cost.one_leg(a, options, stats=(lambda loop: f" demo_stats={loop.demo_stats()}") if bc else None)
    what = f"ExpertLanes({a.lanes}, H = {a.horizon}, S = {a.samples})"
    option_cost.compare(a, __file__, ["off", "expert", "expert+bc"],
                        ["--lanes", str(a.lanes), "--horizon", str(a.horizon), "--samples", str(a.samples), "--bc-weight", str(a.bc_weight)],
                        {"off": "the loop without expert", "expert": what, "expert+bc": f"{what} + DemoLoss({a.bc_weight})"}, 55, records=True)


if __name__ == "__main__":
    main()
