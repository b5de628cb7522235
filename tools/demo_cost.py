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
import option_cost

SIDE = option_cost.SLOTS * option_cost.N // 4


def main():
    a = option_cost.parse([("--bc-weight", dict(type=float, default=1.0)), ("--no-q-filter", dict(action="store_true"))],
                          choices=("off", "on"))
    on = a.leg == "on"

    def options():
        if not on:
            return {}
        from ddpg_trucktrailer_amd.demo_loss import DemoLoss
        return {"demo_loss": DemoLoss(a.bc_weight, not a.no_q_filter)}

    def load_side(loop):
        import torch
        g = torch.Generator().manual_seed(5)
        loop.ring.load_side(torch.rand((SIDE, 23), generator=g) * 2 - 1, torch.rand(SIDE, generator=g) * 2 - 1, torch.randn(SIDE, generator=g),
                            torch.rand((SIDE, 23), generator=g) * 2 - 1, (torch.rand(SIDE, generator=g) < 0.05).to(torch.uint8))

    if a.leg:
        return option_cost.one_leg(a, options, load_side if on else None, (lambda loop: f" demo_stats={loop.demo_stats()}") if on else None)
    option_cost.compare(a, __file__, ["off", "on"], ["--bc-weight", str(a.bc_weight)] + (["--no-q-filter"] if a.no_q_filter else []),
                        dict(off="the loop without demo_loss", on=f"DemoLoss({a.bc_weight}, {not a.no_q_filter}), {SIDE} side tuples"), 40)


if __name__ == "__main__":
    main()
