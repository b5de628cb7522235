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
import option_cost


def main():
    a = option_cost.parse([("--critic", dict(type=float, default=1e4)), ("--actor", dict(type=float, default=1.0))], choices=("off", "on"))
    bounds = (a.critic if a.critic > 0 else None, a.actor if a.actor > 0 else None)

    def options():
        if a.leg == "off":
            return {}
        from ddpg_trucktrailer_amd.grad_clip import GradClip
        return {"grad_clip": GradClip(*bounds)}

    def stats(loop):
        if a.leg == "off":
            return ""
        return "\nCLIP " + "; ".join(f"{k}: clipped {v['clipped']} of {v['updates']}, last norm {v['norm']:.4g}"
                                     for k, v in loop.learner.clip_stats().items())

    if a.leg:
        return option_cost.one_leg(a, options, stats=stats)
    option_cost.compare(a, __file__, ["off", "on"], ["--critic", str(a.critic), "--actor", str(a.actor)],
                        dict(off="the loop without a clip", on=f"GradClip({bounds[0]}, {bounds[1]})"), 28, echo="CLIP ")


if __name__ == "__main__":
    main()
