#!/usr/bin/env python3
"""GPU: what a loss shape costs in the loop, and that a loop without one costs what the parent commit's does.

ms per vector step of DDPGRollout at N = 4096 envs, 64 updates per step, B = 256, graph-replayed (the configuration whose step time
is the learn chain's latency): `legs` legs each of the loop without a shape ("off"), with LossShape(--huber, --pre-penalty) ("on") and,
with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's loop ("parent").  Every leg is a fresh
process; the variants alternate within a round and their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the leg without a shape: its median at most the parent's median plus the parent legs'
own max - min (it launches the parent's kernels: anything else is a host-side regression).  on - off is a record, not a gate.
Usage: loss_shape_cost.py [--legs 3] [--steps 400] [--warmup 60] [--huber 1.0] [--pre-penalty 0.01] [--parent-tree DIR] [--out FILE]
       loss_shape_cost.py --leg off|on [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import option_cost


def main():
    a = option_cost.parse([("--huber", dict(type=float, default=1.0)), ("--pre-penalty", dict(type=float, default=0.01))],
                          choices=("off", "on"))
    shape = (a.huber if a.huber > 0 else None, a.pre_penalty)

    def options():
        if a.leg == "off":
            return {}
        from ddpg_trucktrailer_amd.loss_shape import LossShape
        return {"loss_shape": LossShape(*shape)}

    if a.leg:
        return option_cost.one_leg(a, options)
    option_cost.compare(a, __file__, ["off", "on"], ["--huber", str(a.huber), "--pre-penalty", str(a.pre_penalty)],
                        dict(off="the loop without a shape", on=f"LossShape({shape[0]}, {shape[1]})"), 28)


if __name__ == "__main__":
    main()
