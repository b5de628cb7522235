#!/usr/bin/env python3
"""GPU: what the start-pose curriculum costs in the loop, and that a loop without one costs what the parent commit's does (DESIGN.md
section 37).

ms per vector step of DDPGRollout at --envs lanes (65536: the default loop; 4096) with --updates updates per step, B = 256,
graph-replayed: `legs` legs each of the loop without a curriculum ("off"), with Curriculum(--bins, every=--every) ("on": the
curriculum's step kernel, which adds work for finished lanes only, and one small launch every `every` steps between graph replays)
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's loop ("parent").  Every leg is a
fresh process; the variants alternate within a round and their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the leg without a curriculum: its median at most the parent's median plus the parent
legs' own max - min (it launches the parent's kernels).  on - off is a record, not a gate.
Usage: curriculum_cost.py [--envs 65536] [--updates 1] [--legs 3] [--steps 400] [--warmup 60] [--bins 8,8,8] [--every 64]
                          [--parent-tree DIR] [--out FILE]
       curriculum_cost.py --leg off|on [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import option_cost


def main():
    a = option_cost.parse([("--envs", dict(type=int, default=65536)), ("--updates", dict(type=int, default=1)),
                           ("--bins", dict(default="8,8,8")), ("--every", dict(type=int, default=64))], choices=("off", "on"))
    option_cost.N, option_cost.UPD = a.envs, a.updates
    bins = tuple(int(x) for x in a.bins.split(","))

    def options():
        if a.leg == "off":
            return {}
        from ddpg_trucktrailer_amd.curriculum import Curriculum
        return {"curriculum": Curriculum(bins, every=a.every)}

    def stats(loop):
        if a.leg == "off":
            return ""
        from ddpg_trucktrailer_amd.curriculum import summary
        s = summary(loop.env.curriculum_state())
        return f"\nCURRICULUM cells seen {s['cells_seen']:.3f}, mean p {s['mean_p']:.4f}, top-decile weight {s['top_decile_weight']:.3f}"

    if a.leg:
        return option_cost.one_leg(a, options, stats=stats)
    option_cost.compare(a, __file__, ["off", "on"], ["--envs", str(a.envs), "--updates", str(a.updates), "--bins", a.bins,
                                                     "--every", str(a.every)],
                        dict(off="the loop without a curriculum", on=f"Curriculum({bins}, every={a.every})"), 34, records=True,
                        echo="CURRICULUM ")


if __name__ == "__main__":
    main()
